// ldpc_hip.hip -- C ABI (include/ldpc_hip.h) over the gfx950 kernels in ldpc_kernels.hip.
//
// Host side only: handle lifetime, table upload, workspace carving and the launch
// sequence of one decode.  Nothing here allocates or synchronises inside ldpc_decode
// (graph-capturable); all work goes to the caller's stream.  The host side of the gradient
// path (ldpc_decode_saving, ldpc_backward, ldpc_train_joint*) is ldpc_train_host.hip,
// included below the decode entry points: still this one compiled unit.
#include "ldpc_kernels.hip"
#include "ldpc_resident.hip"
#include "ldpc_train.hip"
#include "ldpc_layered.hip"
#include "ldpc_layered_block.hip"
#include "ldpc_plan.h"

#include <algorithm>
#include <climits>
#include <mutex>
#include <set>
#include <string>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <new>
#include <vector>

#include "../../include/ldpc_hip.h"
#include "../../include/ldpc_hip_debug.h"

using namespace ldpc;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) return fail(LDPC_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_)); \
    } while (0)

constexpr size_t kAlign = 256;
size_t align_up(size_t x) { return (x + kAlign - 1) / kAlign * kAlign; }

template <typename X>
int upload(X **dst, const X *src, size_t count)
{
    *dst = nullptr;
    if (count == 0) count = 1;
    HIP_TRY(hipMalloc((void **)dst, count * sizeof(X)));
    if (src) HIP_TRY(hipMemcpy(*dst, src, count * sizeof(X), hipMemcpyHostToDevice));
    return LDPC_OK;
}

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    explicit DeviceGuard(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (switched) (void)hipSetDevice(prev);
    }
};

}  // namespace

struct ldpc_graph : HostGraph {   // the host copies (ldpc_plan.h) and their device images
    int device = 0;
    int *check_ptr = nullptr, *var_idx = nullptr, *var_ptr = nullptr, *csc_edge = nullptr;
    int *wide_checks = nullptr;    // checks of degree > kWideCheck (cn_sweep_wide splits each over a block)
    int n_wide = 0;
    std::vector<int> h_layer_ptr;  // ldpc_graph_create_layered: [n_layers + 1], validated; empty: the graph declares no layers
    GraphDev dev() const { return GraphDev{n, m, E, check_ptr, var_idx, var_ptr, csc_edge}; }
};

struct ldpc_decoder {
    const ldpc_graph *g = nullptr;
    int dtype = LDPC_F32, form = LDPC_C2V_NMS, T = 0;
    int n_beta = 0, n_alpha = 0, n_levels = 0, n_quant = 0, n_oms_alpha = 0;
    void *beta = nullptr, *alpha = nullptr, *oms_alpha = nullptr;   // device, dtype-typed [T][slots]
    int *beta_slot = nullptr, *alpha_slot = nullptr, *oms_alpha_slot = nullptr;
    float *thresholds = nullptr;   // device [Q][L]
    float *lut = nullptr;          // device [Q][2L] signed reconstruction values
    std::vector<int> q_of_iter;    // host
    int *q_of_iter_dev = nullptr;  // device copy (frozen codewords look their quantiser up)
    std::vector<float> lut_host;   // what `lut` was uploaded from (ldpc_decoder_set_quantizers enqueues the copy)
    int *level_iota = nullptr;     // device 0 .. n_levels: the identity slot map the level gradient is reduced with
    bool resc_per_check = false;   // the compact plan has one beta slot per (sub-)check: its check words follow rcq_zero0
    size_t elem() const { return dtype == LDPC_F64 ? 8 : 4; }
    // LDS-resident engine (ldpc_resident.hip): built at creation when the code qualifies
    int schedule = 0;              // LDPC_SCHED_*
    int mode = 0;                  // LDPC_MODE_*
    bool res_ok = false;
    int res_G = 0, res_NT = 0;
    bool unit_alpha = false, rcq_zero0 = false;   // table properties the resident kernel exploits
    bool beta_per_check = false;                  // every edge of a check uses the same beta slot
    size_t res_lds = 0;
    ResidentPlan res{};
    // compact fixed-T geometry (resident_decode<..., CPT>): a second slot layout at row stride kResCptStride, taken by
    // fixed-T fp32 decodes when three workgroups fit a CU; early-stop and fp64 decodes keep `res`
    bool resc_ok = false;
    size_t resc_lds = 0;
    ResidentPlan resc{};
    CptLayout resc_layout;         // its variable grid and cell table (host copy, ldpc_debug_compact_layout)
    std::vector<void *> res_bufs;  // device allocations owned by the plan
    // inverse slot maps of the gradient path (reduce_table_grads): items of slot s = inv_items[inv_ptr[s] .. inv_ptr[s+1])
    int *beta_inv_ptr = nullptr, *beta_inv_items = nullptr;
    int *alpha_inv_ptr = nullptr, *alpha_inv_items = nullptr;
    int *oms_inv_ptr = nullptr, *oms_inv_items = nullptr;
    // fused RCQ iteration of the streaming engine (cn_gather): per-edge gather metadata, built at creation for fp32
    // flooding RCQ decoders on graphs with variable degree <= 8
    bool gat_ok = false;
    bool pair_ok = false;          // RCQ code-pair form (vn_sweep_q / cn_sweep_q): one beta per check, sorted thresholds
    bool key_float4 = false;       // ... with 4 levels and every threshold 1.. in [2^-50, 2^50]: the float form of the key (kKeyFloat4)
    int4 *gat_meta = nullptr;      // [E + 1]
    int *gat_nbr = nullptr;        // [sum dv(dv-1) + 8]
    // LDS-resident layered decode (ldpc_layered.hip): both layered schedules on codes whose state fits LDS
    bool lay_ok = false;
    LayeredPlan lay{};
    uint32_t *lay_off = nullptr;
    size_t lay_lds = 0;
    int *lay_slot = nullptr;       // LDPC_SCHED_LAYERED: beta slot of each plan entry (-1: none), [m_pad + 2 * kLayPf][lw]
    float *lay_beta = nullptr;     // ... and beta in plan order, [T][m_pad + 2 * kLayPf][lw] (lay_beta_gather)
    bool beta_unit = false;        // every beta is 1.0 (fp32): the layered RCQ kernels skip the weight
    int *lay_oms_slot = nullptr;   // layered offset min-sum: check-side alpha slot of each plan entry, and the table in plan
    float *lay_oms = nullptr;      // order, as lay_slot / lay_beta
    // block-parallel layered decode (ldpc_layered_block.hip): LDPC_SCHED_LAYERED on a graph that declares layers
    bool blk_ok = false;
    std::string blk_why;           // why LDPC_MODE_BLOCK is refused (blk_ok == false)
    BlockPlan blk{};
    size_t blk_lds = 0;
    int blk_threads = 0;
    double blk_mean_layer = 0.0;   // m / L: what the AUTO rule reads
    int *blk_layer_ptr = nullptr, *blk_entry_base = nullptr, *blk_deg = nullptr;
    uint32_t *blk_off = nullptr;
    int *blk_slot = nullptr;       // beta slot of each plan entry (-1: hole), and beta in plan order [T][entries]
    float *blk_beta = nullptr;
    int *blk_oms_slot = nullptr;   // the offset form's check-side alpha, likewise
    float *blk_oms = nullptr;
};

namespace {

// Block-parallel layered kernel: LDPC_MODE_BLOCK forces it.  LDPC_MODE_AUTO would take it when the mean layer size reaches
// kBlkAutoMinMeanLayer.  profiles/block_layered_timing.jsonl (tools/time_block_layered.py, 65536 codewords, T = 10): on one
// base matrix lifted at Z = 1 .. 81 the block kernel first beats the sequential LDS kernel at Z = 16 (1.28x; 3.2x at 32, 5.1x
// at 81, far outside the spread of five repetitions), but on the layer-ordered (1998,1512) graph -- mean layer 24.3, layers of
// 1 .. 40 checks of degree 13-14 -- it loses (NMS 0.98x, W-RCQ 0.57x).  The mean layer size alone does not name the winner,
// so the constant stays "never": AUTO does exactly what it did before and the kernel is reached with LDPC_MODE_BLOCK only.
constexpr double kBlkAutoMinMeanLayer = 1e300;
bool use_block(const ldpc_decoder *d)
{
    return d->blk_ok && (d->mode == LDPC_MODE_BLOCK || (d->mode == LDPC_MODE_AUTO && d->blk_mean_layer >= kBlkAutoMinMeanLayer));
}
bool use_resident(const ldpc_decoder *d) { return d->res_ok && (d->mode == LDPC_MODE_AUTO || d->mode == LDPC_MODE_RESIDENT); }
// layered schedule: the LDS-resident kernel unless a streaming mode is forced (then layered_rcq / layered_minsum, posteriors in HBM)
bool use_layered_lds(const ldpc_decoder *d)
{
    return d->lay_ok && !use_block(d) && (d->mode == LDPC_MODE_AUTO || d->mode == LDPC_MODE_RESIDENT);
}
// streaming engine, RCQ: one fused kernel per iteration (cn_gather) unless the two-sweep form is forced
// streaming forms of an fp32 RCQ decoder, best first: code pair (4E + 4n bytes per iteration), fused gather, two sweeps
bool use_pair(const ldpc_decoder *d) { return d->pair_ok && d->mode != LDPC_MODE_SWEEPS && d->mode != LDPC_MODE_GATHER; }
bool use_gather(const ldpc_decoder *d) { return d->gat_ok && !use_pair(d) && d->mode != LDPC_MODE_SWEEPS && d->mode != LDPC_MODE_PAIR; }

// tile width: 64 lanes x VEC codewords.  fp32: VEC 4 (16 B per lane) for real batches,
// VEC 1 for latency-mode batches <= 64; fp64: VEC 2 / 1.
int pick_vec(const ldpc_decoder *d, int64_t batch)
{
    if (batch <= 64) return 1;
    if (d->schedule != LDPC_SCHED_FLOODING) return 1;      // layered: one dependent chain per wave, as many waves as possible
    return d->dtype == LDPC_F64 ? 2 : 4;
}

// ldpc_decode_capped: the calling thread's decode runs at most this many iterations (INT_MAX outside such a call).  The decode
// entry points only enqueue work, so the cap lives exactly as long as the call that set it.
thread_local int tl_iter_cap = INT_MAX;
inline int capped_T(const ldpc_decoder *d) { return std::min(d->T, tl_iter_cap); }
struct IterCap {
    explicit IterCap(int c) { tl_iter_cap = c; }
    ~IterCap() { tl_iter_cap = INT_MAX; }
};

struct Workspace {
    int vec = 0, tiles = 0;
    char *llrT = nullptr, *v2c = nullptr, *c2v = nullptr, *postT = nullptr;
    char *c2v_prev = nullptr;        // saving forward only: previous iteration's c2v slice (latched rows are carried over)
    uint64_t *bitsT = nullptr, *done = nullptr;
    int *iters = nullptr;
    unsigned long long *unsat = nullptr;     // [tiles][vec] partial syndrome words and
    int *ticket = nullptr;                   // [tiles] block tickets of syndrome_latch_chunks (both zero between launches)
    size_t total = 0;
};

Workspace carve(const ldpc_decoder *d, int64_t batch, void *base)
{
    Workspace w;
    w.vec = pick_vec(d, batch);
    const int W = 64 * w.vec;
    w.tiles = (int)((batch + W - 1) / W);
    if (w.tiles < 1) w.tiles = 1;
    const size_t es = d->elem();
    const size_t n = d->g->n, E = d->g->E, tw = (size_t)w.tiles * W;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        size_t o = off;
        off += align_up(bytes);
        return o;
    };
    const size_t o_llr = take(tw * n * es);
    const size_t o_v2c = take(tw * std::max<size_t>(E, 1) * ((use_gather(d) || use_pair(d)) ? 1 : es));   // gather / code-pair form: the second code buffer
    const size_t o_c2v = take(tw * std::max<size_t>(E, 1) * (d->form == LDPC_C2V_RCQ ? 1 : es));
    const size_t o_post = take(tw * n * es);
    const size_t o_bits = take((size_t)w.tiles * n * w.vec * sizeof(uint64_t));
    const size_t o_done = take((size_t)w.tiles * w.vec * sizeof(uint64_t));
    const size_t o_it = take(tw * sizeof(int));
    const size_t o_unsat = take((size_t)w.tiles * w.vec * sizeof(uint64_t));
    const size_t o_ticket = take((size_t)w.tiles * sizeof(int));
    w.total = off;
    if (base) {
        char *b = (char *)base;
        w.llrT = b + o_llr; w.v2c = b + o_v2c; w.c2v = b + o_c2v; w.postT = b + o_post;
        w.bitsT = (uint64_t *)(b + o_bits); w.done = (uint64_t *)(b + o_done); w.iters = (int *)(b + o_it);
        w.unsat = (unsigned long long *)(b + o_unsat); w.ticket = (int *)(b + o_ticket);
    }
    return w;
}

// ---- launch geometry: the two rules that depend on the tile count -----------------------------
// launch_syndrome / launch_gather launch by them and ldpc_debug_launch_geometry reports them.
// Blocks per tile of the syndrome + latch pass over m checks; 1: the one-block syndrome_latch.
int syndrome_chunks(int m, int tiles)
{
    const int max_chunks = (m + kBlock - 1) / kBlock;
    // 64 tiles or more keep the one-block form (measured equal there: 173 vs 182 us at 128 tiles of the (16200,7200) code)
    return tiles >= 64 ? 1 : std::min(max_chunks, std::max(1, 256 / std::max(tiles, 1)));
}

// Tile mapping of cn_gather on tiles of W codewords: xcd_tiles > 0 the XCD-affine mapping (then == tiles), on a grid padded
// to a multiple of 8 tiles.
struct GatherTiles {
    int xcd_tiles = 0;
    size_t padded = 0;
};
GatherTiles gather_tiles(int n, int E, int tiles, int W)
{
    GatherTiles t;
    // XCD-affine tile mapping when the rows one tile touches (LLRs + both code buffers) fit an XCD's 4 MiB L2: the re-reads
    // then hit there instead of going through the fabric.  At W = 256 that is 4n + 2E <= 16384: neither benchmark code
    // qualifies ((1998,1512): 4n + 2E = 21166; (16200,7200): 29 MB per tile); small_96_48 does, from 16 tiles on.  The
    // figures once quoted here -- (1998,1512) RCQ 6.28 -> 5.85 ms per decode, (16200,7200) 3 % slower -- are those of
    // profiles/r02_ab_timings.json, builds xcd0_vec4 / xcd1_vec4: an A/B build with the mapping forced on for every code,
    // not this condition, under which the (1998,1512) code keeps the tile-major mapping.  No measurement exists under it.
    t.xcd_tiles = (tiles >= 16 && ((size_t)4 * n + 2 * (size_t)E) * W <= (4u << 20)) ? tiles : 0;
    t.padded = t.xcd_tiles ? (size_t)((tiles + 7) / 8) * 8 : (size_t)tiles;
    return t;
}

// ---- launch helpers, one per kernel family ------------------------------------------------
// syndrome + latch: one block per tile when there are many tiles, else `chunks` blocks per tile (syndrome_latch_chunks)
template <int VEC>
void launch_syndrome(const GraphDev &g, const Workspace &w, int it_plus_1, int latch, hipStream_t s)
{
    const int chunks = syndrome_chunks(g.m, w.tiles);
    if (chunks <= 1)
        hipLaunchKernelGGL((syndrome_latch<VEC>), dim3(w.tiles), dim3(kBlock), 0, s, g, w.bitsT, w.done, w.iters, it_plus_1, latch);
    else
        hipLaunchKernelGGL((syndrome_latch_chunks<VEC>), dim3((unsigned)w.tiles * chunks), dim3(kBlock), 0, s, g, w.bitsT, w.done,
                           w.iters, it_plus_1, latch, chunks, w.unsat, w.ticket);
}

template <typename T, int VEC>
int launch_cn(const ldpc_decoder *d, const Workspace &w, int it, bool use_done, hipStream_t s)
{
    const GraphDev g = d->g->dev();
    // small check degrees: two consecutive checks per wave (cn_sweep CPW), for the two forms the benchmarks use
    const int cpw = (g.E < 8 * (long long)g.m && (d->form == LDPC_C2V_NMS || (d->form == LDPC_C2V_RCQ && d->n_levels == 4))) ? 2 : 1;
    const int per_block = kWavesPerBlock * cpw;
    const int cb = (g.m + per_block - 1) / per_block;
    if (cb == 0 || g.E == 0) return LDPC_OK;
    const dim3 grid((unsigned)((size_t)w.tiles * cb)), block(kBlock);
    const bool first = it == 0;
    // > 0: the sweep below skips them, cn_sweep_wide follows.  The sum-product recursion is sequential along a check:
    // cn_sweep keeps checks of every degree, one wave each
    const int n_wide = d->form == LDPC_C2V_SPA ? 0 : d->g->n_wide;
    const T *src = first ? (const T *)w.llrT : (const T *)w.v2c;
    const T *beta_row = (const T *)d->beta + (size_t)it * d->n_beta;
    if constexpr (sizeof(T) == 4 && VEC == 4) {
        // fp32 normalised min-sum on check degrees <= 16: the register-held straight-line form (cn_sweep_f4)
        if (d->form == LDPC_C2V_NMS && d->g->max_dc <= 16 && !w.c2v_prev) {
            const int cb4 = (g.m + kWavesPerBlock - 1) / kWavesPerBlock;
            const dim3 grid4((unsigned)((size_t)w.tiles * cb4));
            const uint64_t *done4 = use_done ? w.done : nullptr;
#define LDPC_CF(FIRST_, BPC_, ES_)                                                                                    \
    hipLaunchKernelGGL((cn_sweep_f4<FIRST_, BPC_, ES_>), grid4, block, 0, s, g, (const float *)src, (float *)w.c2v,     \
                       (const float *)beta_row, (const int *)d->beta_slot, done4, cb4)
            switch ((first ? 4 : 0) + (d->beta_per_check ? 2 : 0) + (done4 ? 1 : 0)) {
            case 0: LDPC_CF(false, false, false); break;
            case 1: LDPC_CF(false, false, true); break;
            case 2: LDPC_CF(false, true, false); break;
            case 3: LDPC_CF(false, true, true); break;
            case 4: LDPC_CF(true, false, false); break;
            case 5: LDPC_CF(true, false, true); break;
            case 6: LDPC_CF(true, true, false); break;
            default: LDPC_CF(true, true, true); break;
            }
#undef LDPC_CF
            HIP_TRY(hipGetLastError());
            return LDPC_OK;
        }
    }
    const T *oa_row = d->oms_alpha ? (const T *)d->oms_alpha + (size_t)it * d->n_oms_alpha : nullptr;
    const float *thr = d->form == LDPC_C2V_RCQ ? d->thresholds + (size_t)d->q_of_iter[it] * d->n_levels : nullptr;
    const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_CN_X(FORM, FIRST, NL_, BPC_, CPW_)                                                                       \
    hipLaunchKernelGGL((cn_sweep<T, VEC, FORM, FIRST, NL_, BPC_, CPW_>), grid, block, 0, s, g, src, (void *)w.c2v,    \
                       beta_row, d->beta_slot, thr, d->n_levels, oa_row, d->oms_alpha_slot, done, cb,             \
                       (const void *)w.c2v_prev, n_wide)
#define LDPC_CN(FORM, FIRST) LDPC_CN_X(FORM, FIRST, 0, false, 1)
    if (d->form == LDPC_C2V_NMS) {
        if (cpw == 2) { if (first) LDPC_CN_X(FORM_NMS, true, 0, false, 2); else LDPC_CN_X(FORM_NMS, false, 0, false, 2); }
        else { if (first) LDPC_CN(FORM_NMS, true); else LDPC_CN(FORM_NMS, false); }
    } else if (d->form == LDPC_C2V_OMS) {
        if (first) LDPC_CN(FORM_OMS, true); else LDPC_CN(FORM_OMS, false);
    } else if (d->form == LDPC_C2V_SPA) {
        if (first) LDPC_CN(FORM_SPA, true); else LDPC_CN(FORM_SPA, false);
    } else {
        if constexpr (sizeof(T) == 4) {
            if (d->n_levels == 4) {                      // bc = 3: compare chain with a compile-time length
                const int variant = (d->beta_per_check ? 2 : 0) + (cpw == 2 ? 1 : 0);
                switch (variant * 2 + (first ? 1 : 0)) {
                case 0: LDPC_CN_X(FORM_RCQ, false, 4, false, 1); break;
                case 1: LDPC_CN_X(FORM_RCQ, true, 4, false, 1); break;
                case 2: LDPC_CN_X(FORM_RCQ, false, 4, false, 2); break;
                case 3: LDPC_CN_X(FORM_RCQ, true, 4, false, 2); break;
                case 4: LDPC_CN_X(FORM_RCQ, false, 4, true, 1); break;
                case 5: LDPC_CN_X(FORM_RCQ, true, 4, true, 1); break;
                case 6: LDPC_CN_X(FORM_RCQ, false, 4, true, 2); break;
                default: LDPC_CN_X(FORM_RCQ, true, 4, true, 2); break;
                }
            } else {
                if (first) LDPC_CN(FORM_RCQ, true); else LDPC_CN(FORM_RCQ, false);
            }
        } else {
            return fail(LDPC_ERR_UNSUPPORTED, "RCQ messages are fp32 only");
        }
    }
#undef LDPC_CN_X
#undef LDPC_CN
    HIP_TRY(hipGetLastError());
    if (n_wide) {
        const dim3 wgrid((unsigned)((size_t)w.tiles * n_wide));
#define LDPC_CW(FORM, FIRST, NL_)                                                                                     \
    hipLaunchKernelGGL((cn_sweep_wide<T, VEC, FORM, FIRST, NL_>), wgrid, block, 0, s, g, (const int *)d->g->wide_checks, \
                       n_wide, src, (void *)w.c2v, beta_row, d->beta_slot, thr, d->n_levels, oa_row,                  \
                       d->oms_alpha_slot, done, (const void *)w.c2v_prev)
        if (d->form == LDPC_C2V_NMS) { if (first) LDPC_CW(FORM_NMS, true, 0); else LDPC_CW(FORM_NMS, false, 0); }
        else if (d->form == LDPC_C2V_OMS) { if (first) LDPC_CW(FORM_OMS, true, 0); else LDPC_CW(FORM_OMS, false, 0); }
        else {
            if constexpr (sizeof(T) == 4) {
                if (d->n_levels == 4) { if (first) LDPC_CW(FORM_RCQ, true, 4); else LDPC_CW(FORM_RCQ, false, 4); }
                else { if (first) LDPC_CW(FORM_RCQ, true, 0); else LDPC_CW(FORM_RCQ, false, 0); }
            }
        }
#undef LDPC_CW
        HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

// where the last variable pass may put the caller's rows itself (vn_last_rows) instead of a tile-major posterior array
struct RowsOut {
    float *posterior = nullptr;
    int32_t *bits = nullptr;
    long long batch = 0;
    int qv = 4;                    // floats per store: 4 / 2 / 1
};

int allow_full_lds(const void *kfn, int device);

// keep_posterior: a non-last sweep also stores the posterior rows in w.postT (fp32 only; ldpc_train_joint and, on the
// code rows of the two-sweep RCQ form, ldpc_train_joint_ste)
template <typename T, int VEC>
int launch_vn(const ldpc_decoder *d, const Workspace &w, int it, bool last, bool use_done, hipStream_t s,
              bool store_posterior = true, const RowsOut *rows = nullptr, bool keep_posterior = false)
{
    const GraphDev g = d->g->dev();
    if constexpr (sizeof(T) == 4 && VEC == 4) {
        if (rows && last) {
            const int row = it < d->T ? it : 0;
            const bool codes = d->form == LDPC_C2V_RCQ;
            const int lut_stride = 2 * d->n_levels;
            const int lut_total = codes ? d->n_quant * lut_stride : 0;
            const int lut_cur = codes ? d->q_of_iter[row] * lut_stride : 0;
            const size_t shmem = vn_rows_stage_bytes() + (size_t)lut_total * sizeof(float);
            const int vb = (g.n + kRowsVars - 1) / kRowsVars;
            const dim3 grid((unsigned)((size_t)w.tiles * rows_grid_chunks(vb, true))), block(kRowsThreads);
            const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_VR(CODES)                                                                                          \
    do {                                                                                                        \
        auto kfn = rows->qv == 4 ? vn_last_rows<CODES, 4> : rows->qv == 2 ? vn_last_rows<CODES, 2> : vn_last_rows<CODES, 1>; \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                              \
        hipLaunchKernelGGL(kfn, grid, block, shmem, s, g, (const void *)w.c2v, (const float *)w.llrT,           \
                           (const float *)d->lut, lut_total, lut_cur, lut_stride, (const int *)d->q_of_iter_dev, \
                           (const int *)w.iters, w.bitsT, done, rows->posterior, rows->bits, rows->batch, vb);  \
    } while (0)
            if (codes) LDPC_VR(true); else LDPC_VR(false);
#undef LDPC_VR
            HIP_TRY(hipGetLastError());
            return LDPC_OK;
        }
    }
    const int vb = (g.n + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 grid((unsigned)((size_t)w.tiles * vb)), block(kBlock);
    const int row = it < d->T ? it : 0;     // T == 0: posterior-only pass, alpha unused
    const T *alpha_row = (const T *)d->alpha + (size_t)row * d->n_alpha;
    const bool codes = d->form == LDPC_C2V_RCQ;
    const int lut_stride = 2 * d->n_levels;
    const int lut_total = codes ? d->n_quant * lut_stride : 0;
    const int lut_cur = codes ? d->q_of_iter[row] * lut_stride : 0;
    const size_t shmem = (size_t)lut_total * sizeof(float);
    const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_VN(CODES, LAST, ...)                                                                      \
    hipLaunchKernelGGL((vn_sweep<T, VEC, CODES, LAST, ##__VA_ARGS__>), grid, block, shmem, s, g, (const void *)w.c2v,  \
                       (const T *)w.llrT, (T *)w.v2c, alpha_row, d->alpha_slot, (const float *)d->lut,  \
                       lut_total, lut_cur, lut_stride, (const int *)d->q_of_iter_dev,                   \
                       (const int *)w.iters, w.bitsT, store_posterior ? (T *)w.postT : (T *)nullptr, done, vb)
    if (codes) {
        if constexpr (sizeof(T) == 4) {
            if (last) LDPC_VN(true, true); else if (keep_posterior) LDPC_VN(true, false, true); else LDPC_VN(true, false);
        } else {
            return fail(LDPC_ERR_UNSUPPORTED, "RCQ messages are fp32 only");
        }
    } else if (keep_posterior && !last) {
        if constexpr (sizeof(T) == 4) LDPC_VN(false, false, true);
        else return fail(LDPC_ERR_UNSUPPORTED, "internal: posterior-keeping sweeps are fp32 only");
    } else {
        if (last) LDPC_VN(false, true); else LDPC_VN(false, false);
    }
#undef LDPC_VN
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// code-pair form, iterations >= 1: V2C codes (w.v2c) -> C2V codes (w.c2v)
template <int VEC>
int launch_cn_q(const ldpc_decoder *d, const Workspace &w, int it, bool use_done, hipStream_t s)
{
    const GraphDev g = d->g->dev();
    const int dmax = d->g->max_dc;
    const int cpw = (dmax <= 8 && g.E < 8 * (long long)g.m) ? 2 : 1;
    const int per_block = kWavesPerBlock * cpw;
    const int cb = (g.m + per_block - 1) / per_block;
    if (cb == 0 || g.E == 0) return LDPC_OK;
    const dim3 grid((unsigned)((size_t)w.tiles * cb)), block(kBlock);
    const float *beta_row = (const float *)d->beta + (size_t)it * d->n_beta;
    const float *thr = d->thresholds + (size_t)d->q_of_iter[it] * d->n_levels;
    const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_CQ(CPW_, DCMAX_)                                                                                        \
    hipLaunchKernelGGL((cn_sweep_q<VEC, CPW_, DCMAX_>), grid, block, 0, s, g, (const uint8_t *)w.v2c, (uint8_t *)w.c2v, \
                       beta_row, (const int *)d->beta_slot, thr, d->n_levels, done, cb)
#define LDPC_CQ4(CPW_, DCMAX_)                                                                                       \
    do {                                                                                                             \
        if (done)                                                                                                    \
            hipLaunchKernelGGL((cn_sweep_q4<CPW_, DCMAX_, true>), grid, block, 0, s, g, (const uint8_t *)w.v2c,       \
                               (uint8_t *)w.c2v, beta_row, (const int *)d->beta_slot, d->n_levels, done, cb);        \
        else                                                                                                         \
            hipLaunchKernelGGL((cn_sweep_q4<CPW_, DCMAX_, false>), grid, block, 0, s, g, (const uint8_t *)w.v2c,      \
                               (uint8_t *)w.c2v, beta_row, (const int *)d->beta_slot, d->n_levels, done, cb);        \
    } while (0)
    if constexpr (VEC == 4) {
        if (dmax <= 8) { if (cpw == 2) LDPC_CQ4(2, 8); else LDPC_CQ4(1, 8); }
        else if (dmax <= 16) LDPC_CQ4(1, 16);
        else if (dmax <= 32) LDPC_CQ4(1, 32);
        else LDPC_CQ4(1, 0);
    } else {
        if (dmax <= 8) { if (cpw == 2) LDPC_CQ(2, 8); else LDPC_CQ(1, 8); }
        else if (dmax <= 16) LDPC_CQ(1, 16);
        else if (dmax <= 32) LDPC_CQ(1, 32);
        else LDPC_CQ(1, 0);
    }
#undef LDPC_CQ4
#undef LDPC_CQ
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// 256-codeword tiles of a decoder whose variable sweep can run vn_sweep_q4 (degrees <= 8, at most 8 levels)
template <int VEC>
bool pair_q4(const ldpc_decoder *d) { return VEC == 4 && d->g->max_dv <= 8 && d->n_levels <= 8; }

// code-pair form, iterations < T-1: C2V codes of iteration `it` (w.c2v) -> V2C codes for iteration it + 1 (w.v2c).
// it == -1 (pair_q4 decoders only): the pass before iteration 0, LLRs -> V2C codes for iteration 0.
template <int VEC>
int launch_vn_q(const ldpc_decoder *d, const Workspace &w, int it, bool use_done, hipStream_t s)
{
    const bool init = it < 0;
    if (init) it = 0;
    const GraphDev g = d->g->dev();
    const int vb = (g.n + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 grid((unsigned)((size_t)w.tiles * vb)), block(kBlock);
    const float *alpha_row = (const float *)d->alpha + (size_t)it * d->n_alpha;
    const int nxt = init ? 0 : it + 1;
    const float *beta_next = (const float *)d->beta + (size_t)nxt * d->n_beta;
    const float *thr_next = d->thresholds + (size_t)d->q_of_iter[nxt] * d->n_levels;
    const int lut_entries = 2 * d->n_levels;
    const float *lut_cur = d->lut + (size_t)d->q_of_iter[it] * lut_entries;
    const size_t shmem = (size_t)lut_entries * sizeof(float);
    const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_VQ(NL_)                                                                                                  \
    hipLaunchKernelGGL((vn_sweep_q<VEC, NL_>), grid, block, shmem, s, g, (const uint8_t *)w.c2v, (const float *)w.llrT, \
                       (uint8_t *)w.v2c, alpha_row, (const int *)d->alpha_slot, lut_cur, lut_entries, beta_next,        \
                       (const int *)d->beta_slot, thr_next, d->n_levels, w.bitsT, done, vb)
    const int vb4 = (g.n + kWavesPerBlock * kVnqVpw - 1) / (kWavesPerBlock * kVnqVpw);
    const dim3 grid4((unsigned)((size_t)w.tiles * vb4));
#define LDPC_VQ4(NL_, ES_)                                                                                            \
    hipLaunchKernelGGL((vn_sweep_q4<NL_, ES_, kVnqVpw>), grid4, block, shmem, s, g, (const uint8_t *)w.c2v,         \
                       (const float *)w.llrT, (uint8_t *)w.v2c, alpha_row, (const int *)d->alpha_slot, lut_cur,         \
                       lut_entries, beta_next, (const int *)d->beta_slot, thr_next, d->n_levels, w.bitsT, done, vb4)
    if (init) {
        if (!pair_q4<VEC>(d)) return fail(LDPC_ERR_ARG, "internal: code-pair initial pass on a decoder without vn_sweep_q4");
#define LDPC_VQI(NL_)                                                                                                 \
    hipLaunchKernelGGL((vn_sweep_q4<NL_, false, kVnqVpw, true>), grid4, block, 0, s, g, (const uint8_t *)w.c2v,     \
                       (const float *)w.llrT, (uint8_t *)w.v2c, alpha_row, (const int *)d->alpha_slot, lut_cur,         \
                       lut_entries, beta_next, (const int *)d->beta_slot, thr_next, d->n_levels, w.bitsT, done, vb4)
        if (d->key_float4) LDPC_VQI(kKeyFloat4); else if (d->n_levels == 4) LDPC_VQI(4); else LDPC_VQI(0);
#undef LDPC_VQI
    } else if (pair_q4<VEC>(d)) {
        if (d->key_float4) { if (done) LDPC_VQ4(kKeyFloat4, true); else LDPC_VQ4(kKeyFloat4, false); }
        else if (d->n_levels == 4) { if (done) LDPC_VQ4(4, true); else LDPC_VQ4(4, false); }
        else { if (done) LDPC_VQ4(0, true); else LDPC_VQ4(0, false); }
    }
    else if (d->n_levels == 4) LDPC_VQ(4); else LDPC_VQ(0);
#undef LDPC_VQ4
#undef LDPC_VQ
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// fused RCQ iteration `it` >= 1: codes of iteration it-1 (`cin`) -> codes of iteration it (`cout`)
template <int VEC>
int launch_gather(const ldpc_decoder *d, const Workspace &w, int it, bool use_done, const char *cin, char *cout,
                  hipStream_t s)
{
    const GraphDev g = d->g->dev();
    const int cpw = (g.E < 8 * (long long)g.m) ? 2 : 1;
    const int per_block = kWavesPerBlock * cpw;
    const int cb = (g.m + per_block - 1) / per_block;
    if (cb == 0 || g.E == 0) return LDPC_OK;
    const GatherTiles gt = gather_tiles(g.n, g.E, w.tiles, 64 * VEC);       // XCD-affine mapping or tile-major
    const int xcd_tiles = gt.xcd_tiles;
    const dim3 grid((unsigned)(gt.padded * cb)), block(kBlock);
    const float *beta_row = (const float *)d->beta + (size_t)it * d->n_beta;
    const float *alpha_prev = (const float *)d->alpha + (size_t)(it - 1) * d->n_alpha;
    const float *thr = d->thresholds + (size_t)d->q_of_iter[it] * d->n_levels;
    const int lut_entries = 2 * d->n_levels;
    const float *lut_prev = d->lut + (size_t)d->q_of_iter[it - 1] * lut_entries;     // the quantiser that produced `cin`
    const size_t shmem = (size_t)lut_entries * sizeof(float);
    const uint64_t *done = use_done ? w.done : nullptr;
#define LDPC_GA(NL_, BPC_, CPW_)                                                                                     \
    hipLaunchKernelGGL((cn_gather<VEC, NL_, BPC_, CPW_, kGatherGrp>), grid, block, shmem, s, g,                  \
                       (const int4 *)d->gat_meta, (const int *)d->gat_nbr, (const float *)w.llrT, (const uint8_t *)cin, \
                       (uint8_t *)cout, beta_row, (const int *)d->beta_slot, alpha_prev, thr, d->n_levels, lut_prev,   \
                       lut_entries, done, cb, xcd_tiles)
    const int variant = (d->n_levels == 4 ? 4 : 0) + (d->beta_per_check ? 2 : 0) + (cpw == 2 ? 1 : 0);
    switch (variant) {
    case 0: LDPC_GA(0, false, 1); break;
    case 1: LDPC_GA(0, false, 2); break;
    case 2: LDPC_GA(0, true, 1); break;
    case 3: LDPC_GA(0, true, 2); break;
    case 4: LDPC_GA(4, false, 1); break;
    case 5: LDPC_GA(4, false, 2); break;
    case 6: LDPC_GA(4, true, 1); break;
    default: LDPC_GA(4, true, 2); break;
    }
#undef LDPC_GA
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// Saved forward state of the training path: c2v rows of iterations 0..T-1, then the v2c input rows of
// iterations 1..T-1 (iteration 0 reads the LLRs), each slice [tile][E][W] fp32.
struct SavedLayout {
    size_t slice = 0;
    int T = 0;
    size_t c2v_off(int it) const { return (size_t)it * slice; }
    size_t v2c_off(int it) const { return ((size_t)T + (size_t)(it - 1)) * slice; }      // it >= 1
    size_t total() const { return T > 0 ? (size_t)(2 * T - 1) * slice : 0; }
};
SavedLayout saved_layout(const ldpc_decoder *d, int tiles, int W)
{
    SavedLayout sl;
    sl.T = d->T;
    sl.slice = align_up((size_t)tiles * W * std::max(d->g->E, 1) * sizeof(float));
    return sl;
}

// vector forms of the layout changes: the caller side moves the widest of 16 / 8 / 4 bytes per lane that divides the row
// length in bytes and that both pointers are aligned to (NULL counts as aligned), never less than one element.  0: the
// scalar kernels -- an fp64 decoder whose `bits` sit at 4 mod 8 (a legal int32_t*), or a pointer below its element's alignment
int vec_bytes(size_t elem, int n, const void *a, const void *b)
{
    for (int vb = 16; vb >= (int)elem; vb >>= 1)
        if (((size_t)n * elem) % vb == 0 && ((uintptr_t)a & (vb - 1)) == 0 && ((uintptr_t)b & (vb - 1)) == 0) return vb;
    return 0;
}

// The kernels that move a streaming decode's rows between the caller's layout and the tiles, chosen from the tile width,
// the row length and the addresses of the caller's pointers (compared, never dereferenced).  decode_impl launches by this
// and ldpc_debug_boundary_kernels reports it.
enum { kOutNone = 0, kOutLayout = 1, kOutLastRows = 2 };
struct BoundaryKernels {
    int vec = 0;
    int in_bytes = 0;        // caller-side bytes per access of the entrance pass (transpose_in_v / transpose_in_q4); 0: transpose_in
    bool fused_in = false;   // code-pair form on 256-codeword tiles: the entrance pass also codes the LLRs (transpose_in_q4)
    int out_path = kOutNone; // kOutLayout: transpose_out_v / transpose_out; kOutLastRows: vn_last_rows stores the caller's rows
    int out_bytes = 0;       // caller-side bytes per access on the way out (vn_last_rows: 4 * QV); 0: transpose_out
};
BoundaryKernels boundary_kernels(const ldpc_decoder *d, int vec, int T_it, bool saving, const void *llr,
                                 const void *posterior, const int32_t *bits)
{
    const size_t elem = d->elem();
    // fp32 flooding decode on 256-codeword tiles outside the training forward: the fused passes at either end may run
    const bool rows4 = elem == 4 && vec == 4 && d->schedule == LDPC_SCHED_FLOODING && !saving && T_it > 0;
    BoundaryKernels k;
    k.vec = vec;
    k.in_bytes = vec_bytes(elem, d->g->n, llr, nullptr);
    k.fused_in = rows4 && use_pair(d) && pair_q4<4>(d) && k.in_bytes == 16;
    if (bits || posterior) {
        k.out_bytes = vec_bytes(elem, d->g->n, posterior, bits);
        k.out_path = rows4 && k.out_bytes >= 4 ? kOutLastRows : kOutLayout;
    }
    return k;
}

template <typename T, int VEC>
int decode_impl(const ldpc_decoder *d, const void *llr, int64_t batch, bool early_stop, int32_t *bits,
                void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed,
                const Workspace &w, hipStream_t s, char *saved = nullptr)
{
    constexpr int W = 64 * VEC;
    constexpr int JT = transpose_vars<T>();
    const GraphDev g = d->g->dev();
    const int T_it = capped_T(d);
    const bool need_post = bits || posterior;          // packed decisions / iterations only: the last pass stores no posterior rows
    const int vc = (g.n + JT - 1) / JT;
    const dim3 tgrid((unsigned)((size_t)w.tiles * VEC * vc));       // transposes: one block per (tile, 64-codeword run, chunk)
    const BoundaryKernels bk = boundary_kernels(d, VEC, T_it, saved != nullptr, llr, posterior, bits);

    auto layout_in = [&]() {
        switch (bk.in_bytes) {
        case 16: hipLaunchKernelGGL((transpose_in_v<T, VEC, 16>), tgrid, dim3(kBlock), 0, s, (const T *)llr, (T *)w.llrT, (long long)batch, g.n, vc); break;
        case 8: hipLaunchKernelGGL((transpose_in_v<T, VEC, 8>), tgrid, dim3(kBlock), 0, s, (const T *)llr, (T *)w.llrT, (long long)batch, g.n, vc); break;
        case 4:
            if constexpr (sizeof(T) == 4) {
                hipLaunchKernelGGL((transpose_in_v<T, VEC, 4>), tgrid, dim3(kBlock), 0, s, (const T *)llr, (T *)w.llrT, (long long)batch, g.n, vc);
                break;
            }
            [[fallthrough]];
        default: hipLaunchKernelGGL((transpose_in<T, VEC>), tgrid, dim3(kBlock), 0, s, (const T *)llr, (T *)w.llrT, (long long)batch, g.n, vc);
        }
    };
    auto layout_out = [&](const T *srcT) {
        switch (bk.out_bytes) {
        case 16: hipLaunchKernelGGL((transpose_out_v<T, VEC, 16>), tgrid, dim3(kBlock), 0, s, srcT, w.bitsT, (T *)posterior, bits, (long long)batch, g.n, vc); break;
        case 8: hipLaunchKernelGGL((transpose_out_v<T, VEC, 8>), tgrid, dim3(kBlock), 0, s, srcT, w.bitsT, (T *)posterior, bits, (long long)batch, g.n, vc); break;
        case 4:
            if constexpr (sizeof(T) == 4) {
                hipLaunchKernelGGL((transpose_out_v<T, VEC, 4>), tgrid, dim3(kBlock), 0, s, srcT, w.bitsT, (T *)posterior, bits, (long long)batch, g.n, vc);
                break;
            }
            [[fallthrough]];
        default: hipLaunchKernelGGL((transpose_out<T, VEC>), tgrid, dim3(kBlock), 0, s, srcT, w.bitsT, (T *)posterior, bits, (long long)batch, g.n, vc);
        }
    };
    // code-pair form on 256-codeword tiles: the layout change also codes the LLRs for iteration 0 (transpose_in_q4)
    const bool fused_init = bk.fused_in;
    if constexpr (sizeof(T) == 4 && VEC == 4) {
        if (fused_init) {
            const int vb = (g.n + kRowsVars - 1) / kRowsVars;
            const float *beta0 = (const float *)d->beta;
            const float *thr0 = d->thresholds + (size_t)d->q_of_iter[0] * d->n_levels;
#define LDPC_TIQ(NL_)                                                                                                \
    do {                                                                                                             \
        auto kfn = transpose_in_q4<NL_>;                                                                             \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                   \
        hipLaunchKernelGGL(kfn, dim3((unsigned)((size_t)w.tiles * rows_grid_chunks(vb, false))), dim3(kRowsThreads), vn_rows_stage_bytes(), s, g, \
                           (const float *)llr, (float *)w.llrT, (uint8_t *)w.v2c, beta0, (const int *)d->beta_slot, \
                           thr0, d->n_levels, (long long)batch, vb);                                                \
    } while (0)
            if (d->key_float4) LDPC_TIQ(kKeyFloat4); else if (d->n_levels == 4) LDPC_TIQ(4); else LDPC_TIQ(0);
#undef LDPC_TIQ
        }
    }
    if (!fused_init) layout_in();
    {
        const long long cnt = (long long)w.tiles * W;
        hipLaunchKernelGGL((init_state<VEC>), dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, w.done,
                           w.iters, (long long)batch, w.tiles, T_it, w.unsat, w.ticket);
    }
    HIP_TRY(hipGetLastError());

    if (d->schedule != LDPC_SCHED_FLOODING) {
        if constexpr (sizeof(T) == 4) {
            // posteriors start as the LLRs and are updated in place, check after check, by one wave per tile;
            // LDPC_SCHED_LAYERED keeps every edge's message code in the c2v buffer (subtracted before the check's update)
            if (d->form != LDPC_C2V_RCQ) {
                // the min-sum forms keep the message itself (fp32 per edge); "no message yet" is +0
                HIP_TRY(hipMemsetAsync(w.c2v, 0, (size_t)w.tiles * W * std::max(g.E, 1) * sizeof(float), s));
                if (d->form == LDPC_C2V_NMS)
                    hipLaunchKernelGGL((layered_minsum<VEC, FORM_NMS>), dim3(w.tiles), dim3(kWave), 0, s, g, (float *)w.llrT,
                                       (float *)w.c2v, (const float *)d->beta, d->beta_slot, d->n_beta, (const float *)nullptr,
                                       (const int *)nullptr, 0, T_it, early_stop ? 1 : 0, w.bitsT, w.done, w.iters);
                else
                    hipLaunchKernelGGL((layered_minsum<VEC, FORM_OMS>), dim3(w.tiles), dim3(kWave), 0, s, g, (float *)w.llrT,
                                       (float *)w.c2v, (const float *)d->beta, d->beta_slot, d->n_beta,
                                       (const float *)d->oms_alpha, d->oms_alpha_slot, d->n_oms_alpha, T_it,
                                       early_stop ? 1 : 0, w.bitsT, w.done, w.iters);
            } else if (d->schedule == LDPC_SCHED_LAYERED)
                hipLaunchKernelGGL((layered_rcq<VEC, true>), dim3(w.tiles), dim3(kWave), 0, s, g, (float *)w.llrT, d->thresholds,
                                   d->n_levels, (const int *)d->q_of_iter_dev, T_it, early_stop ? 1 : 0, w.bitsT, w.done, w.iters,
                                   d->g->max_dc, (uint8_t *)w.c2v, d->beta_unit ? nullptr : (const float *)d->beta,
                                   d->beta_slot, d->n_beta);
            else
                hipLaunchKernelGGL((layered_rcq<VEC, false>), dim3(w.tiles), dim3(kWave), 0, s, g, (float *)w.llrT, d->thresholds,
                                   d->n_levels, (const int *)d->q_of_iter_dev, T_it, early_stop ? 1 : 0, w.bitsT, w.done, w.iters,
                                   d->g->max_dc, (uint8_t *)nullptr, nullptr, nullptr, 0);
            HIP_TRY(hipGetLastError());
            if (early_stop && T_it == 0) HIP_TRY(hipMemsetAsync(w.done, 0, (size_t)w.tiles * VEC * sizeof(uint64_t), s));
            if (bits || posterior) layout_out((const T *)w.llrT);
            if (iterations || success || packed) {
                long long threads = batch;
                if (packed) threads = std::max<long long>(threads, std::min<long long>(batch * ((g.n + 7) / 8), 1ll << 22));
                hipLaunchKernelGGL((finalize_out<VEC>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, w.done,
                                   w.iters, w.bitsT, iterations, success, packed, (long long)batch, g.n);
            }
            HIP_TRY(hipGetLastError());
            return LDPC_OK;
        } else {
            return fail(LDPC_ERR_UNSUPPORTED, "layered schedule is fp32 only");
        }
    }
    // fp32, 256-codeword tiles: the last variable pass writes posterior / decisions into the caller's rows itself
    // (vn_last_rows, 4 / 2 / 1 floats per store) -- no tile-major posterior array, no transpose_out pass
    RowsOut rows_out;
    const RowsOut *rows = nullptr;
    if constexpr (sizeof(T) == 4 && VEC == 4) {
        if (bk.out_path == kOutLastRows) {
            rows_out.posterior = (float *)posterior; rows_out.bits = bits; rows_out.batch = (long long)batch;
            rows_out.qv = bk.out_bytes / 4;
            rows = &rows_out;
        }
    }
    if (T_it == 0) {
        // no iteration ran: c2v == 0, posterior = llr + 0  (loop skipped, ldpc_decoder.py:147-153)
        const size_t c2v_bytes = (size_t)w.tiles * W * std::max(g.E, 1) * (d->form == LDPC_C2V_RCQ ? 1 : sizeof(T));
        HIP_TRY(hipMemsetAsync(w.c2v, 0, c2v_bytes, s));
        int rc = launch_vn<T, VEC>(d, w, 0, /*last=*/true, /*use_done=*/false, s);
        if (rc) return rc;
    }
    if (use_pair(d) && !saved) {
        if constexpr (sizeof(T) == 4) {
            // RCQ, code-pair form: both directions are 1-byte codes (iteration 0 of decoders without vn_sweep_q4 is the plain
            // check sweep on the LLRs) (vn_sweep_q quantises with the next iteration's beta and thresholds, cn_sweep_q is integer-only);
            // the last variable pass is the ordinary posterior pass over the C2V codes.
            const bool q4 = pair_q4<VEC>(d);      // LLRs -> V2C codes first, then iteration 0 is a code sweep like the others
            if (q4 && T_it > 0 && !fused_init) {
                int rc = launch_vn_q<VEC>(d, w, -1, false, s);
                if (rc) return rc;
            }
            for (int it = 0; it < T_it; ++it) {
                int rc = (it == 0 && !q4) ? launch_cn<T, VEC>(d, w, 0, early_stop, s) : launch_cn_q<VEC>(d, w, it, early_stop, s);
                if (rc) return rc;
                rc = it == T_it - 1 ? launch_vn<T, VEC>(d, w, it, /*last=*/true, early_stop, s, /*store_posterior=*/need_post, rows)
                                    : launch_vn_q<VEC>(d, w, it, early_stop, s);
                if (rc) return rc;
                if (early_stop)
                    launch_syndrome<VEC>(g, w, it + 1, 1, s);
            }
        }
    } else if (use_gather(d) && !saved) {
        if constexpr (sizeof(T) == 4) {
            // RCQ, fused form: iteration 0 is the plain check sweep on the LLRs, every later iteration ONE cn_gather
            // launch (codes ping-pong between the two code buffers; iteration `it` writes buffer it & 1).  The hard
            // decisions the stop rule needs come from a posterior-only variable pass per iteration (early stop), or
            // once at the end (fixed T).
            char *buf[2] = {w.c2v, w.v2c};
            for (int it = 0; it < T_it; ++it) {
                int rc;
                if (it == 0) {
                    rc = launch_cn<T, VEC>(d, w, 0, early_stop, s);
                } else {
                    rc = launch_gather<VEC>(d, w, it, early_stop, buf[(it - 1) & 1], buf[it & 1], s);
                }
                if (rc) return rc;
                const bool last = it == T_it - 1;
                if (early_stop || last) {
                    Workspace wv = w;
                    wv.c2v = buf[it & 1];
                    rc = launch_vn<T, VEC>(d, wv, it, /*last=*/true, early_stop, s, /*store_posterior=*/last && need_post, last ? rows : nullptr);
                    if (rc) return rc;
                }
                if (early_stop)
                    launch_syndrome<VEC>(g, w, it + 1, 1, s);
            }
        }
    } else
    for (int it = 0; it < T_it; ++it) {
        // training forward: iteration `it` writes its c2v rows, and the v2c rows the next one reads, straight into
        // their slices of `saved` (SavedLayout).  A stopped codeword's rows stay latched because the check sweep
        // carries them over from the previous slice -- the final variable sweep forms its posterior from them.
        Workspace wc = w, wv = w;
        if (saved) {
            const SavedLayout sl = saved_layout(d, w.tiles, W);
            wc.c2v = wv.c2v = saved + sl.c2v_off(it);
            if (it > 0) {
                wc.v2c = saved + sl.v2c_off(it);
                if (early_stop) wc.c2v_prev = saved + sl.c2v_off(it - 1);
            }
            if (it + 1 < T_it) wv.v2c = saved + sl.v2c_off(it + 1);
        }
        int rc = launch_cn<T, VEC>(d, wc, it, early_stop, s);
        if (rc) return rc;
        rc = launch_vn<T, VEC>(d, wv, it, it == T_it - 1, early_stop, s, /*store_posterior=*/it == T_it - 1 ? need_post : true, rows);
        if (rc) return rc;
        if (early_stop) {
            launch_syndrome<VEC>(g, w, it + 1, 1, s);
        }
    }
    if (!early_stop) {
        launch_syndrome<VEC>(g, w, T_it, 0, s);
    } else if (T_it == 0) {
        // reference: the loop never ran, success False, iterations 0 -> clear the (padding) latch bits
        HIP_TRY(hipMemsetAsync(w.done, 0, (size_t)w.tiles * VEC * sizeof(uint64_t), s));
    }
    HIP_TRY(hipGetLastError());

    if ((bits || posterior) && !rows) layout_out((const T *)w.postT);
    if (iterations || success || packed) {
        long long threads = batch;
        if (packed) threads = std::max<long long>(threads, std::min<long long>(batch * ((g.n + 7) / 8), 1ll << 22));
        hipLaunchKernelGGL((finalize_out<VEC>), dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, w.done,
                           w.iters, w.bitsT, iterations, success, packed, (long long)batch, g.n);
    }
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

template <typename T>
int decode_dispatch(const ldpc_decoder *d, const void *llr, int64_t batch, bool early_stop, int32_t *bits,
                    void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed,
                    const Workspace &w, hipStream_t s, char *saved = nullptr)
{
    switch (w.vec) {
    case 1: return decode_impl<T, 1>(d, llr, batch, early_stop, bits, posterior, iterations, success, packed, w, s, saved);
    case 2:
        if constexpr (sizeof(T) == 8)
            return decode_impl<T, 2>(d, llr, batch, early_stop, bits, posterior, iterations, success, packed, w, s, saved);
        break;
    case 4:
        if constexpr (sizeof(T) == 4)
            return decode_impl<T, 4>(d, llr, batch, early_stop, bits, posterior, iterations, success, packed, w, s, saved);
        break;
    }
    return fail(LDPC_ERR_ARG, "internal: bad tile width");
}


// Everything the decoder derives from the VALUES of its quantiser tables, in one place: ldpc_decoder_create and
// ldpc_decoder_set_quantizers both go through quantizer_flags / apply_quantizer_flags, so a decoder whose thresholds were
// replaced picks the kernels a freshly created one would.
struct QuantizerFlags {
    bool pair_ok = false;       // code-pair form: thresholds 1.. of every quantiser positive and non-decreasing
    bool key_float4 = false;    // ... 4 levels, every one of them in [2^-50, 2^50]: the float form of the key
    bool rcq_zero0 = false;     // every tau_0 == 0: the resident kernel quantises per check (and the compact plan's check words)
    bool lay_zero0 = false;     // layered plans: magnitude 0 reconstructs to 0 under every quantiser
    bool lay_sorted = false;    // layered plans: tau_1 <= tau_2 <= ... under every quantiser
};

QuantizerFlags quantizer_flags(const ldpc_decoder *d, const float *thr)
{
    QuantizerFlags f;
    const int L = d->n_levels, Q = d->n_quant;
    const ldpc_graph *g = d->g;
    if (d->dtype == LDPC_F32 && d->schedule == LDPC_SCHED_FLOODING && g->E > 0 && d->beta_per_check && L <= 62) {
        // code-pair form: level(|beta * x|) must be non-decreasing in x, i.e. thresholds 1.. of every quantiser sorted, and
        // positive (level(0) = 0; the magnitude compares run on the bit patterns)
        // (threshold 0 never decides a level, rcq_decoder.py:79-85)
        bool sorted = true;
        for (int q = 0; q < Q && sorted; ++q)
            for (int k = 1; k < L; ++k) {
                const float t = thr[(size_t)q * L + k];
                if (!(t > 0.0f) || (k > 1 && t < thr[(size_t)q * L + k - 1])) { sorted = false; break; }
            }
        f.pair_ok = sorted;
        bool in_range = sorted && L == 4;
        for (int q = 0; q < Q && in_range; ++q)
            for (int k = 1; k < L; ++k) {
                const float t = thr[(size_t)q * L + k];
                if (!(t >= 0x1p-50f && t <= 0x1p50f)) in_range = false;
            }
        f.key_float4 = in_range;
    }
    f.rcq_zero0 = true;
    for (int q = 0; q < Q; ++q) f.rcq_zero0 = f.rcq_zero0 && thr[(size_t)q * L] == 0.0f;
    // magnitude 0 reconstructs to 0 under every quantiser (rcq_decoder.py:79-85, :107-119): tau_0 == 0 and no later
    // threshold <= 0 -- true for the reference's C * (j / (2^(bc-1) - 1))^gamma with gamma > 0
    f.lay_zero0 = true;
    for (int q = 0; q < Q; ++q) {
        float rec = thr[(size_t)q * L];
        for (int k = 1; k < L; ++k)
            if (0.0f >= thr[(size_t)q * L + k]) rec = thr[(size_t)q * L + k];
        f.lay_zero0 = f.lay_zero0 && rec == 0.0f;
    }
    f.lay_sorted = true;                                              // tau_1 <= tau_2 <= ... under every quantiser
    for (int q = 0; q < Q; ++q)
        for (int k = 2; k < L; ++k) f.lay_sorted = f.lay_sorted && thr[(size_t)q * L + k - 1] <= thr[(size_t)q * L + k];
    return f;
}

// the flags into the decoder and into the plans already built from earlier ones (creation: none yet, the plan builders
// read d->rcq_zero0 and call quantizer_flags themselves)
void apply_quantizer_flags(ldpc_decoder *d, const QuantizerFlags &f)
{
    d->pair_ok = f.pair_ok; d->key_float4 = f.key_float4; d->rcq_zero0 = f.rcq_zero0;
    if (d->resc_ok) {                                 // compact plan: which waves run the scalar-counted check phase
        std::vector<ResVCheck> vc;
        if (resident_checks(d->g, vc)) cpt_check_words(vc, d->resc_per_check && f.rcq_zero0, d->resc.ccell);
    }
    if (d->lay_ok) { d->lay.zero0 = f.lay_zero0 ? 1 : 0; d->lay.sorted = f.lay_sorted ? 1 : 0; }
}

// signed reconstruction LUT: value of code c = (1 - 2*sign_bit) * tau[c mod L]  (rcq_decoder.py:107-119)
void fill_quantizer_lut(ldpc_decoder *d, const float *thr)
{
    const size_t L = d->n_levels, Q = d->n_quant;
    d->lut_host.resize(Q * 2 * L);
    for (size_t q = 0; q < Q; ++q)
        for (size_t c = 0; c < 2 * L; ++c) {
            const float sb = c >= L ? 1.0f : 0.0f;
            d->lut_host[q * 2 * L + c] = (1.0f - 2.0f * sb) * thr[q * L + (c % L)];
        }
}

// alpha table identically 1.0f: an exact shortcut in the resident kernel (the quantiser's flags: quantizer_flags)
void resident_table_flags(ldpc_decoder *d, const void *alpha_host)
{
    if (alpha_host) {
        const size_t cnt = (size_t)std::max(d->T, 0) * d->n_alpha;
        bool unit = true;
        if (d->dtype == LDPC_F32) {
            const float *a = (const float *)alpha_host;
            for (size_t k = 0; k < cnt; ++k) unit = unit && a[k] == 1.0f;
        } else {
            const double *a = (const double *)alpha_host;
            for (size_t k = 0; k < cnt; ++k) unit = unit && a[k] == 1.0;
        }
        d->unit_alpha = unit;
    }
}

// every beta is 1.0: the layered schedules then run their unweighted form (same results, no weight loads)
void beta_table_flags(ldpc_decoder *d, const void *beta_host)
{
    bool unit = d->dtype == LDPC_F32;
    const size_t cnt = (size_t)std::max(d->T, 0) * d->n_beta;
    for (size_t k = 0; k < cnt && unit; ++k) unit = ((const float *)beta_host)[k] == 1.0f;
    d->beta_unit = unit;
}

// ---- LDS-resident engine: plan upload (the planner is ldpc_plan.h) ------------------------------
static_assert(kPlanF32 == LDPC_F32 && kPlanF64 == LDPC_F64 && kPlanNMS == LDPC_C2V_NMS && kPlanRCQ == LDPC_C2V_RCQ &&
              kPlanOMS == LDPC_C2V_OMS, "the planner's dtype and form values are the C ABI's");
static_assert(sizeof(Word2) == sizeof(uint2) && alignof(Word2) <= alignof(uint2) && offsetof(Word2, x) == offsetof(uint2, x) &&
              offsetof(Word2, y) == offsetof(uint2, y), "Word2 tables are uploaded as uint2");

template <typename X, typename H>
int plan_upload(ldpc_decoder *d, const X **dst, const std::vector<H> &src)
{
    static_assert(sizeof(X) == sizeof(H), "host and device element");
    X *p = nullptr;
    int rc = upload(&p, reinterpret_cast<const X *>(src.data()), src.size());
    if (rc) return rc;
    d->res_bufs.push_back((void *)p);
    *dst = p;
    return LDPC_OK;
}

// one planned geometry to the device: the scalars into pl, the tables into allocations owned by d->res_bufs
int upload_plan(ldpc_decoder *d, const PlanTables &t, ResidentPlan &pl)
{
    pl = ResidentPlan{};
    pl.n = t.n; pl.m = t.m; pl.S = t.S; pl.max_dc = t.max_dc; pl.max_dv = t.max_dv; pl.mstride = t.mstride; pl.E = t.E;
    pl.any_split = t.any_split; pl.par_words = t.par_words; pl.par_shift = t.par_shift;
    pl.n_hi = t.n_hi; pl.n_pos = t.n_pos;
    std::copy(t.vcell, t.vcell + 8, pl.vcell);
    std::copy(t.ccell, t.ccell + 8, pl.ccell);
    int rc = plan_upload(d, &pl.dc_s, t.dc_s);
    if (!rc && t.any_split) rc = plan_upload(d, &pl.gsz, t.gsz);
    if (!rc) rc = plan_upload(d, &pl.cvar, t.cvar);
    if (!rc) rc = plan_upload(d, &pl.bslot, t.bslot);
    if (!rc && t.per_check) rc = plan_upload(d, &pl.bslot_c, t.bslot_c);
    if (!rc && t.has_oaslot) rc = plan_upload(d, &pl.oaslot, t.oaslot);
    if (!rc) rc = plan_upload(d, &pl.vmeta, t.vmeta);
    if (!rc) rc = plan_upload(d, &pl.vslot_lo, t.vslot_lo);
    if (!rc) rc = plan_upload(d, &pl.vslot_hi, t.vslot_hi);
    if (!rc) rc = plan_upload(d, &pl.inv_perm_v, t.inv_perm_v);
    if (!rc) rc = plan_upload(d, &pl.edge_of_slot, t.edge_of_slot);
    return rc;
}

PlanInputs plan_inputs(const ldpc_decoder *d, const ldpc_decoder_desc *desc)
{
    PlanInputs in;
    in.dtype = d->dtype; in.form = d->form; in.T = d->T;
    in.n_beta = d->n_beta; in.n_alpha = d->n_alpha; in.n_oms_alpha = d->n_oms_alpha;
    in.beta_per_check = d->beta_per_check; in.rcq_zero0 = d->rcq_zero0;
    in.has_oms_alpha = desc->oms_alpha != nullptr;
    in.beta_slot = desc->beta_slot; in.alpha_slot = desc->alpha_slot; in.oms_alpha_slot = desc->oms_alpha_slot;
    return in;
}

int build_resident_plan(ldpc_decoder *d, const ldpc_decoder_desc *desc)
{
    ResidentChoice c = choose_resident_plan(d->g, plan_inputs(d, desc));
    d->res_ok = d->resc_ok = false;
    if (!c.res_ok) return LDPC_OK;
    if (int rc = upload_plan(d, c.res, d->res)) return rc;
    d->res_G = c.G; d->res_NT = c.NT; d->res_lds = c.res_lds;
    d->res_ok = true;
    if (!c.resc_ok) return LDPC_OK;
    if (int rc = upload_plan(d, c.resc, d->resc)) return rc;
    d->resc_layout = std::move(c.resc_layout);
    d->resc_lds = c.resc_lds;
    d->resc_per_check = c.resc.per_check;
    d->resc_ok = true;
    return LDPC_OK;
}

// A kernel's dynamic-LDS ceiling is process-wide state of that kernel on a device: it is raised ONCE per
// instantiation and device to the full 160 KiB (not per launch, and not to one decoder's size -- another decoder
// of a larger code launches the same instantiation).
int allow_full_lds(const void *kfn, int device)
{
    static std::mutex mu;
    static std::set<std::pair<const void *, int>> done;
    std::lock_guard<std::mutex> lk(mu);
    if (done.count({kfn, device})) return LDPC_OK;
    HIP_TRY(hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBytes));
    done.insert({kfn, device});
    return LDPC_OK;
}

// the variable state fits the lanes' registers (ResVarState): at most kResRegVars variables per lane, every degree > 4
// variable in the first round, no split checks; other codes keep the streaming variable loop.  Fixed-T decodes only:
// the early-stop kernels carry the syndrome/emit state as well and would spill the register state to scratch
bool resident_reg_state(const ldpc_decoder *d)
{
    return !d->res.any_split && d->res.n <= kResRegVars * d->res_NT && d->res.n_hi <= d->res_NT;
}

// What a decode of d launches on the LDS-resident engine in stop mode `early_stop`: the plan and the template arguments
// of resident_decode.  The ONE place that holds these predicates: launch_resident switches on the fields, and
// ldpc_debug_resident_kernel reports them.
enum { kResPlanGeneral = 0, kResPlanReg = 1, kResPlanCompact = 2 };
struct ResidentKernel {
    int plan;            // kResPlanGeneral: streaming variable loop; kResPlanReg: register-held variable state (d->res);
                         // kResPlanCompact: the compact fixed-T geometry (d->resc)
    int G, form, nl, ms; // template arguments of the KERNEL: codewords per workgroup, FORM_*, NL and MS (0: the run-time value).
                         // G is 1 for fp64 although the host dispatch is launch_resident<2> (the plan's geometry is a float
                         // pair's); the launcher does not read it, only the hook reports it
    bool bpc, split, f64;
    bool alpha_in_lds;   // ResidentArgs::alpha_in_lds of the launch
};

ResidentKernel resident_kernel(const ldpc_decoder *d, bool early_stop)
{
    ResidentKernel k{};
    const bool reg = resident_reg_state(d) && !early_stop;
    k.form = d->form == LDPC_C2V_NMS ? FORM_NMS : d->form == LDPC_C2V_OMS ? FORM_OMS : FORM_RCQ;
    k.f64 = d->dtype == LDPC_F64;
    k.alpha_in_lds = resident_alpha_floats(d->dtype, d->T, d->n_alpha) > 0;
    if (d->resc_ok && !early_stop) {   // compact fixed-T geometry, three workgroups per CU (resc_ok implies fp32 and G = 2)
        k.plan = kResPlanCompact;
        k.G = 2;
        k.bpc = d->resc.bslot_c != nullptr;
        k.nl = (k.form == FORM_RCQ && d->n_levels == 4) ? 4 : 0;
        k.ms = kResCptStride;
        k.alpha_in_lds = false;                       // no alpha table in the compact carve: read from global memory
        return k;
    }
    // codes with split (wide) checks run the generic instantiation (run-time stride and level count) with the lane-group
    // exchange compiled in -- the specialised ones stay exactly as lean as without the feature
    k.G = k.f64 ? 1 : d->res_G;                       // one fp64 codeword per workgroup in the slots of a float pair
    k.bpc = d->res.bslot_c != nullptr;
    k.split = d->res.any_split != 0;
    k.ms = (!k.split && d->res.mstride == 512) ? 512 : 0;
    k.nl = (!k.split && k.form == FORM_RCQ && d->n_levels == 4) ? 4 : 0;   // bc = 3, the paper's and the benchmark's quantiser
    k.plan = (!k.split && reg) ? kResPlanReg : kResPlanGeneral;
    return k;
}

template <int G>
int launch_resident(const ldpc_decoder *d, const ResidentArgs &args, hipStream_t s)
{
    const size_t lds = d->res_lds;
    const ResidentKernel k = resident_kernel(d, args.early_stop);
    const bool reg = k.plan == kResPlanReg;
    ResidentArgs a = args;
    a.alpha_in_lds = k.alpha_in_lds;
    if (k.f64) {
        if (G != 2 || !k.bpc) return fail(LDPC_ERR_ARG, "internal: fp64 resident geometry");
        const unsigned blocks64 = (unsigned)a.batch;
#define LDPC_RES64(MS, SPLIT, REG)                                                                        \
    do {                                                                                                  \
        auto kfn = a.early_stop ? resident_decode<1, FORM_NMS, true, 0, MS, 1, double, SPLIT, false>      \
                                : resident_decode<1, FORM_NMS, true, 0, MS, 0, double, SPLIT, REG>;       \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                        \
        hipLaunchKernelGGL(kfn, dim3(blocks64), dim3(d->res_NT), lds, s, d->res, a);                      \
    } while (0)
        if (k.split) LDPC_RES64(0, true, false);
        else if (k.ms == 512) { if (reg) LDPC_RES64(512, false, true); else LDPC_RES64(512, false, false); }
        else if (reg) LDPC_RES64(0, false, true);
        else LDPC_RES64(0, false, false);
#undef LDPC_RES64
        HIP_TRY(hipGetLastError());
        return LDPC_OK;
    }
    const unsigned blocks = (unsigned)((a.batch + G - 1) / G);
    if constexpr (G == 2) {
        if (k.plan == kResPlanCompact) {
#define LDPC_RES_CPT(FORM, NL)                                                                                         \
    do {                                                                                                               \
        auto kfn = k.bpc ? resident_decode<2, FORM, true, NL, kResCptStride, 0, float, false, true, true>              \
                         : resident_decode<2, FORM, false, NL, kResCptStride, 0, float, false, true, true>;            \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                     \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kResCptThreads), d->resc_lds, s, d->resc, a);                       \
    } while (0)
            if (k.form == FORM_NMS) LDPC_RES_CPT(FORM_NMS, 0);
            else if (k.form == FORM_OMS) LDPC_RES_CPT(FORM_OMS, 0);
            else if (k.nl == 4) LDPC_RES_CPT(FORM_RCQ, 4);
            else LDPC_RES_CPT(FORM_RCQ, 0);
#undef LDPC_RES_CPT
            HIP_TRY(hipGetLastError());
            return LDPC_OK;
        }
    }
#define LDPC_RES_MS(FORM, NL, MS, SPLIT, REG)                                                            \
    do {                                                                                                 \
        auto kfn = k.bpc ? (a.early_stop ? resident_decode<G, FORM, true, NL, MS, 1, float, SPLIT, false>            \
                                         : resident_decode<G, FORM, true, NL, MS, 0, float, SPLIT, REG>)             \
                         : (a.early_stop ? resident_decode<G, FORM, false, NL, MS, 1, float, SPLIT, false>           \
                                         : resident_decode<G, FORM, false, NL, MS, 0, float, SPLIT, REG>);           \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                       \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(d->res_NT), lds, s, d->res, a);                       \
    } while (0)
#define LDPC_RES(FORM, NL)                                                                               \
    do {                                                                                                 \
        if (k.split) LDPC_RES_MS(FORM, 0, 0, true, false);                                               \
        else if (k.ms == 512) {                                                                          \
            if (reg) LDPC_RES_MS(FORM, NL, 512, false, true);                                            \
            else LDPC_RES_MS(FORM, NL, 512, false, false);                                               \
        } else if (reg) LDPC_RES_MS(FORM, NL, 0, false, true);                                           \
        else LDPC_RES_MS(FORM, NL, 0, false, false);                                                     \
    } while (0)
    if (k.form == FORM_NMS) LDPC_RES(FORM_NMS, 0);
    else if (k.form == FORM_OMS) LDPC_RES(FORM_OMS, 0);
    else if (k.nl == 4) LDPC_RES(FORM_RCQ, 4);
    else LDPC_RES(FORM_RCQ, 0);
#undef LDPC_RES_MS
#undef LDPC_RES
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int decode_resident(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t *bits,
                    void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed_bits, void *dbg_c2v,
                    void *stream)
{
    DeviceGuard guard(d->g->device);
    ResidentArgs a{};
    a.llr = (const float *)llr; a.batch = batch; a.T = capped_T(d); a.early_stop = early_stop != 0;
    a.beta = (const float *)d->beta; a.n_beta = d->n_beta;
    a.alpha = (const float *)d->alpha; a.n_alpha = d->n_alpha;
    a.oms_alpha = (const float *)d->oms_alpha; a.n_oms_alpha = d->n_oms_alpha;
    a.thr = d->thresholds; a.n_levels = d->n_levels; a.q_of_iter = d->q_of_iter_dev;
    a.bits = bits; a.posterior = (float *)posterior; a.iterations = iterations; a.success = success;
    a.packed = packed_bits;
    a.dbg_c2v = dbg_c2v;
    a.unit_alpha = d->unit_alpha; a.rcq_zero0 = d->rcq_zero0;
    hipStream_t rs = (hipStream_t)stream;
    switch (d->res_G) {
    case 1: return launch_resident<1>(d, a, rs);
    default: return launch_resident<2>(d, a, rs);
    }
}

// ---- LDS-resident layered decode: plan (host) and launch -----------------------------------------------------
// LDPC_SCHED_LAYERED: the decoder's beta table in plan order (d->lay_beta), enqueued on `s` after the table's upload
int gather_layered_beta(const ldpc_decoder *d, hipStream_t s)
{
    if (!d->lay_beta || d->T == 0) return LDPC_OK;
    const int entries = (d->lay.m_pad + 2 * kLayPf) * d->lay.lw;
    const long long cnt = (long long)entries * d->T;
    hipLaunchKernelGGL(lay_beta_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const float *)d->beta, d->n_beta,
                       (const int *)d->lay_slot, entries, d->T, d->lay_beta);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}
// layered offset min-sum: the check-side alpha table in plan order (d->lay_oms), likewise
int gather_layered_oms(const ldpc_decoder *d, hipStream_t s)
{
    if (!d->lay_oms || d->T == 0) return LDPC_OK;
    const int entries = (d->lay.m_pad + 2 * kLayPf) * d->lay.lw;
    const long long cnt = (long long)entries * d->T;
    hipLaunchKernelGGL(lay_beta_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const float *)d->oms_alpha,
                       d->n_oms_alpha, (const int *)d->lay_oms_slot, entries, d->T, d->lay_oms);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

constexpr size_t kLayPaperMinWaves = 4;           // LDPC_SCHED_LAYERED takes the LDS kernel only with a wave per SIMD
int build_layered_plan(ldpc_decoder *d, const ldpc_decoder_desc *desc)
{
    const ldpc_graph *g = d->g;
    d->lay_ok = false;
    if (d->schedule == LDPC_SCHED_FLOODING || d->dtype != LDPC_F32) return LDPC_OK;
    if (g->E == 0 || g->m == 0 || g->max_dc > 64) return LDPC_OK;     // a check wider than a wavefront: streaming kernel
    const bool paper = d->schedule == LDPC_SCHED_LAYERED;
    const bool minsum = d->form != LDPC_C2V_RCQ;                      // layered_minsum_lds: check records in place of the codes
    int lw = 1;
    while (lw < g->max_dc) lw <<= 1;
    const int m_pad = (g->m + kLayPf - 1) / kLayPf * kLayPf;
    // LDPC_SCHED_LAYERED also keeps one code byte per plan entry of the codeword's walk after its posteriors
    const size_t code_off = lay_row_bytes(g->n);
    // ... the min-sum forms one record per plan row: 16 bytes up to 32 lanes, 24 at 64 (ldpc_layered.hip)
    const size_t row_bytes = minsum ? code_off + (size_t)m_pad * (lw <= 32 ? 16 : 24)
                             : paper ? code_off + ((size_t)m_pad * lw + 3) / 4 * 4 : lay_row_bytes(g->n);
    int cw = 64 / lw;
    while (cw > 1 && (size_t)cw * row_bytes > kLdsBytes) cw >>= 1;
    if ((size_t)cw * row_bytes > kLdsBytes) return LDPC_OK;           // one codeword's state exceeds LDS
    if (paper) {
        // the codes make a codeword's state large: a full wave of codewords may leave SIMDs without a wave ((1998,1512):
        // 4 x 15.8 KB -> two workgroups per CU).  Take the codewords per wave that put the most codewords on a CU, the
        // fuller wave on a tie (4 -> 8, 3 -> 9, 2 -> 10, 1 -> 10 codewords per CU there).
        int best = cw, best_cu = 0;
        for (int c = cw; c >= 1; --c) {
            const int per_cu = c * (int)(kLdsBytes / ((size_t)c * row_bytes));
            if (per_cu > best_cu) { best = c; best_cu = per_cu; }
        }
        cw = best;
        // fewer than one wave per SIMD loses to the streaming kernel: (16200,7200) keeps one 137 KB codeword per CU and ran
        // 3.5x slower than layered_rcq (1872 vs 528 ms at 32768 codewords, T = 10) -- it stays on the streaming kernel
        if (kLdsBytes / ((size_t)cw * row_bytes) < kLayPaperMinWaves) return LDPC_OK;
    }
    if ((size_t)g->n * 4u + 4u > kLayOffMask) return LDPC_OK;
    const uint32_t none = (uint32_t)g->n * 4u;                        // the codeword's +inf word
    std::vector<uint32_t> off((size_t)(m_pad + 2 * kLayPf) * lw, none);
    bool deg1 = false;
    // edges right-aligned in ascending variable order: the last lane holds the highest variable of the check
    auto var_at = [&](int row, int t) -> int {                       // variable in lane t of plan row `row`, -1: none
        if (row >= g->m) return -1;
        const int e0 = g->h_check_ptr[row], dc = g->h_check_ptr[row + 1] - e0, k = t - (lw - dc);
        return k >= 0 ? g->h_var_idx[e0 + k] : -1;
    };
    for (int i = 0; i < m_pad; ++i) {
        const int dc = i < g->m ? g->h_check_ptr[i + 1] - g->h_check_ptr[i] : 0;
        deg1 = deg1 || dc == 1;
        for (int t = 0; t < lw; ++t) {
            const int v = var_at(i, t);
            const uint32_t o = v >= 0 ? (uint32_t)v * 4u : none;
            off[(size_t)i * lw + t] = o | (dc == 1 ? kLayDeg1Bit : 0u);
        }
    }
    // what the kernels may assume of the quantiser tables (quantizer_flags; both hold trivially for the min-sum forms)
    const QuantizerFlags qf = minsum ? QuantizerFlags{} : quantizer_flags(d, desc->thresholds);
    const bool zero0 = minsum || qf.lay_zero0, sorted = minsum || qf.lay_sorted;
    int rc = upload(&d->lay_off, off.data(), off.size());
    if (rc) return rc;
    // A power-of-two region per codeword (address = offset | row bits, one v_and_or_b32) was measured and dropped: 4 x 8192 bytes
    // leave room for only four workgroups per CU instead of five and put the four rows of a wave on the same LDS banks
    // ((1998,1512): 11.2 vs 9.6 ms, profiles/r03_layered_variants.txt).  The kernel keeps the template flag for A/B builds.
    const int row_shift = 0;
    d->lay = LayeredPlan{g->n, g->m, lw, cw, m_pad, deg1 ? 1 : 0, zero0 ? 1 : 0, sorted ? 1 : 0, row_shift, d->lay_off,
                         (unsigned)row_bytes, (unsigned)code_off, nullptr, nullptr};
    d->lay_lds = row_shift ? ((size_t)cw << row_shift) : (size_t)cw * row_bytes;
    if (paper) {
        // beta of every plan entry, per iteration: gathered on the device from the decoder's table (again on set_weights)
        std::vector<int> slot((size_t)(m_pad + 2 * kLayPf) * lw, -1);
        for (int i = 0; i < g->m; ++i) {
            const int e0 = g->h_check_ptr[i], dc = g->h_check_ptr[i + 1] - e0;
            for (int k = 0; k < dc; ++k) slot[(size_t)i * lw + (lw - dc) + k] = desc->beta_slot[e0 + k];
        }
        rc = upload(&d->lay_slot, slot.data(), slot.size());
        if (!rc) rc = upload(&d->lay_beta, (const float *)nullptr, slot.size() * (size_t)std::max(d->T, 1));
        if (!rc) rc = gather_layered_beta(d, nullptr);
        if (!rc && minsum && d->oms_alpha) {
            // the offset form's check-side alpha, the same way
            std::fill(slot.begin(), slot.end(), -1);
            for (int i = 0; i < g->m; ++i) {
                const int e0 = g->h_check_ptr[i], dc = g->h_check_ptr[i + 1] - e0;
                for (int k = 0; k < dc; ++k) slot[(size_t)i * lw + (lw - dc) + k] = desc->oms_alpha_slot[e0 + k];
            }
            rc = upload(&d->lay_oms_slot, slot.data(), slot.size());
            if (!rc) rc = upload(&d->lay_oms, (const float *)nullptr, slot.size() * (size_t)std::max(d->T, 1));
            if (!rc) rc = gather_layered_oms(d, nullptr);
        }
        if (!rc) HIP_TRY(hipStreamSynchronize(nullptr));
        if (rc) return rc;
        d->lay.beta_lay = d->lay_beta;
        d->lay.oms_lay = d->lay_oms;
    }
    d->lay_ok = true;
    return LDPC_OK;
}

int decode_layered_lds(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t *bits,
                       void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed_bits, void *stream)
{
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const LayeredPlan &pl = d->lay;
    const unsigned blocks = (unsigned)((batch + pl.cw - 1) / pl.cw);
    if (d->form != LDPC_C2V_RCQ) {
#define LDPC_LMS_K(LW_, FORM_, ES_, OA_)                                                                             \
    do {                                                                                                             \
        auto kfn = layered_minsum_lds<LW_, FORM_, ES_, OA_>;                                                         \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                   \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kWave), d->lay_lds, s, pl, (const float *)llr, (long long)batch, \
                           capped_T(d), bits, (float *)posterior, iterations, success, packed_bits);                \
    } while (0)
#define LDPC_LMS_LW(LW_)                                                                                             \
    do {                                                                                                             \
        if (d->form == LDPC_C2V_NMS) { if (early_stop) LDPC_LMS_K(LW_, FORM_NMS, true, false); else LDPC_LMS_K(LW_, FORM_NMS, false, false); } \
        else if (pl.oms_lay) { if (early_stop) LDPC_LMS_K(LW_, FORM_OMS, true, true); else LDPC_LMS_K(LW_, FORM_OMS, false, true); } \
        else { if (early_stop) LDPC_LMS_K(LW_, FORM_OMS, true, false); else LDPC_LMS_K(LW_, FORM_OMS, false, false); } \
    } while (0)
        switch (pl.lw) {
        case 1: LDPC_LMS_LW(1); break;
        case 2: LDPC_LMS_LW(2); break;
        case 4: LDPC_LMS_LW(4); break;
        case 8: LDPC_LMS_LW(8); break;
        case 16: LDPC_LMS_LW(16); break;
        case 32: LDPC_LMS_LW(32); break;
        default: LDPC_LMS_LW(64); break;
        }
#undef LDPC_LMS_LW
#undef LDPC_LMS_K
        HIP_TRY(hipGetLastError());
        return LDPC_OK;
    }
    if (d->schedule == LDPC_SCHED_LAYERED) {
#define LDPC_PAP_K(LW_, NL_, ES_, WB_)                                                                               \
    do {                                                                                                             \
        auto kfn = layered_paper_lds<LW_, NL_, ES_, WB_>;                                                            \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                   \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kWave), d->lay_lds, s, pl, (const float *)llr, (long long)batch, \
                           (const float *)d->thresholds, d->n_levels, (const int *)d->q_of_iter_dev, capped_T(d),   \
                           bits, (float *)posterior, iterations, success, packed_bits);                             \
    } while (0)
#define LDPC_PAP_NL(LW_, ES_, WB_)                                                                                   \
    do {                                                                                                             \
        if (d->n_levels == 4) LDPC_PAP_K(LW_, 4, ES_, WB_); else LDPC_PAP_K(LW_, 0, ES_, WB_);                      \
    } while (0)
#define LDPC_PAP_LW(LW_)                                                                                             \
    do {                                                                                                             \
        if (early_stop) { if (d->beta_unit) LDPC_PAP_NL(LW_, true, false); else LDPC_PAP_NL(LW_, true, true); }       \
        else { if (d->beta_unit) LDPC_PAP_NL(LW_, false, false); else LDPC_PAP_NL(LW_, false, true); }                \
    } while (0)
        switch (pl.lw) {
        case 1: LDPC_PAP_LW(1); break;
        case 2: LDPC_PAP_LW(2); break;
        case 4: LDPC_PAP_LW(4); break;
        case 8: LDPC_PAP_LW(8); break;
        case 16: LDPC_PAP_LW(16); break;
        case 32: LDPC_PAP_LW(32); break;
        default: LDPC_PAP_LW(64); break;
        }
#undef LDPC_PAP_LW
#undef LDPC_PAP_NL
#undef LDPC_PAP_K
        HIP_TRY(hipGetLastError());
        return LDPC_OK;
    }
#define LDPC_LAY_K(LW_, NL_, ES_, D1_, Z0_, SO_)                                                                     \
    do {                                                                                                             \
        auto kfn = pl.row_shift ? layered_lds<LW_, NL_, ES_, D1_, Z0_, SO_, true> : layered_lds<LW_, NL_, ES_, D1_, Z0_, SO_, false>; \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                   \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kWave), d->lay_lds, s, pl, (const float *)llr, (long long)batch, \
                           (const float *)d->thresholds, d->n_levels, (const int *)d->q_of_iter_dev, capped_T(d),   \
                           bits, (float *)posterior, iterations, success, packed_bits);                             \
    } while (0)
    // the common case (bc = 3, no degree-1 check, zero reconstructs to zero) gets the lean instantiation per stop mode;
    // everything else the general one (run-time level count, degree-1 flag, the reference's "w < 0" sign test)
#define LDPC_LAY_NL(LW_)                                                                                             \
    do {                                                                                                             \
        const bool lean = d->n_levels == 4 && !pl.has_deg1 && pl.zero0 && pl.sorted;                                 \
        if (lean) { if (early_stop) LDPC_LAY_K(LW_, 4, true, false, true, true); else LDPC_LAY_K(LW_, 4, false, false, true, true); } \
        else { if (early_stop) LDPC_LAY_K(LW_, 0, true, true, false, false); else LDPC_LAY_K(LW_, 0, false, true, false, false); } \
    } while (0)
    switch (pl.lw) {
    case 1: LDPC_LAY_NL(1); break;
    case 2: LDPC_LAY_NL(2); break;
    case 4: LDPC_LAY_NL(4); break;
    case 8: LDPC_LAY_NL(8); break;
    case 16: LDPC_LAY_NL(16); break;
    case 32: LDPC_LAY_NL(32); break;
    default: LDPC_LAY_NL(64); break;
    }
#undef LDPC_LAY_NL
#undef LDPC_LAY_K
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// ---- block-parallel layered decode: plan (ldpc_layer_plan.h) and launch -------------------------------------------
// the decoder's beta table (and the offset form's check-side alpha) in plan order, enqueued on `s` after the table's upload
int gather_block_tables(const ldpc_decoder *d, bool beta, bool oms, hipStream_t s)
{
    if (!d->blk_ok || d->T == 0) return LDPC_OK;
    const int entries = d->blk.entries;
    const long long cnt = (long long)entries * d->T;
    if (beta && d->blk_beta) {
        hipLaunchKernelGGL(lay_beta_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const float *)d->beta, d->n_beta,
                           (const int *)d->blk_slot, entries, d->T, d->blk_beta);
        HIP_TRY(hipGetLastError());
    }
    if (oms && d->blk_oms) {
        hipLaunchKernelGGL(lay_beta_gather, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const float *)d->oms_alpha,
                           d->n_oms_alpha, (const int *)d->blk_oms_slot, entries, d->T, d->blk_oms);
        HIP_TRY(hipGetLastError());
    }
    return LDPC_OK;
}

int build_block_plan(ldpc_decoder *d, const ldpc_decoder_desc *desc)
{
    const ldpc_graph *g = d->g;
    d->blk_ok = false;
    if (g->h_layer_ptr.empty()) { d->blk_why = "the graph declares no layers (ldpc_graph_create_layered)"; return LDPC_OK; }
    if (d->dtype != LDPC_F32) { d->blk_why = "the block-parallel layered kernel is fp32 only"; return LDPC_OK; }
    if (d->schedule != LDPC_SCHED_LAYERED) { d->blk_why = "the block-parallel kernel runs LDPC_SCHED_LAYERED only"; return LDPC_OK; }
    if (d->form == LDPC_C2V_SPA) { d->blk_why = "the sum-product form has no layered schedule"; return LDPC_OK; }
    const bool rcq = d->form == LDPC_C2V_RCQ;
    const int L = (int)g->h_layer_ptr.size() - 1;
    LayerPlan p = layer_plan(g->n, g->m, g->h_check_ptr.data(), g->h_var_idx.data(), L, g->h_layer_ptr.data(),
                             rcq ? kBlkRcq : kBlkMinSum);
    if (!p.ok) { d->blk_why = p.why; return LDPC_OK; }
    int rc = upload(&d->blk_layer_ptr, p.layer_ptr.data(), p.layer_ptr.size());
    if (!rc) rc = upload(&d->blk_entry_base, p.entry_base.data(), p.entry_base.size());
    if (!rc) rc = upload(&d->blk_deg, p.deg.data(), p.deg.size());
    if (!rc) rc = upload(&d->blk_off, p.off.data(), p.off.size());
    std::vector<int> slot((size_t)p.entries, -1);
    for (int k = 0; k < p.entries; ++k)
        if (p.edge_of_entry[k] >= 0) slot[k] = desc->beta_slot[p.edge_of_entry[k]];
    if (!rc) rc = upload(&d->blk_slot, slot.data(), slot.size());
    if (!rc) rc = upload(&d->blk_beta, (const float *)nullptr, slot.size() * (size_t)std::max(d->T, 1));
    if (!rc && d->form == LDPC_C2V_OMS && d->oms_alpha) {
        for (int k = 0; k < p.entries; ++k)
            if (p.edge_of_entry[k] >= 0) slot[k] = desc->oms_alpha_slot[p.edge_of_entry[k]];
        rc = upload(&d->blk_oms_slot, slot.data(), slot.size());
        if (!rc) rc = upload(&d->blk_oms, (const float *)nullptr, slot.size() * (size_t)std::max(d->T, 1));
    }
    if (rc) return rc;
    d->blk = BlockPlan{p.n, p.m, p.L, p.W, p.G, p.lpc, p.row_words, p.rec_off, p.entries, d->blk_layer_ptr, d->blk_entry_base,
                       d->blk_deg, d->blk_off, d->blk_beta, d->blk_oms};
    d->blk_lds = p.lds_bytes;
    d->blk_threads = p.threads;
    d->blk_mean_layer = (double)p.m / (double)p.L;
    d->blk_ok = true;
    rc = gather_block_tables(d, true, true, nullptr);
    if (!rc) HIP_TRY(hipStreamSynchronize(nullptr));
    return rc;
}

int decode_block(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t *bits,
                 void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed_bits, void *stream)
{
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const BlockPlan &pl = d->blk;
    const unsigned blocks = (unsigned)((batch + pl.G - 1) / pl.G);
#define LDPC_BLK_K(FORM_, ES_, AUX_)                                                                                 \
    do {                                                                                                             \
        auto kfn = layered_block_lds<FORM_, ES_, AUX_>;                                                              \
        if (int rc_ = allow_full_lds((const void *)kfn, d->g->device)) return rc_;                                   \
        hipLaunchKernelGGL(kfn, dim3(blocks), dim3((unsigned)d->blk_threads), d->blk_lds, s, pl, (const float *)llr, \
                           (long long)batch, (const float *)d->thresholds, d->n_levels, (const int *)d->q_of_iter_dev, \
                           capped_T(d), bits, (float *)posterior, iterations, success, packed_bits);                \
    } while (0)
#define LDPC_BLK_ES(FORM_, AUX_)                                                                                     \
    do {                                                                                                             \
        if (early_stop) LDPC_BLK_K(FORM_, true, AUX_); else LDPC_BLK_K(FORM_, false, AUX_);                          \
    } while (0)
    if (d->form == LDPC_C2V_RCQ) { if (d->beta_unit) LDPC_BLK_ES(FORM_RCQ, false); else LDPC_BLK_ES(FORM_RCQ, true); }
    else if (d->form == LDPC_C2V_NMS) LDPC_BLK_ES(FORM_NMS, false);
    else if (pl.oms_lay) LDPC_BLK_ES(FORM_OMS, true);
    else LDPC_BLK_ES(FORM_OMS, false);
#undef LDPC_BLK_ES
#undef LDPC_BLK_K
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

}  // namespace

// =========================================================================================== C ABI
extern "C" {

const char *ldpc_last_error(void) { return g_err; }
int ldpc_abi_version(void) { return LDPC_HIP_ABI_VERSION; }
#ifndef LDPC_SRC_HASH
#define LDPC_SRC_HASH unknown
#endif
#define LDPC_STR2(x) #x
#define LDPC_STR(x) LDPC_STR2(x)
const char *ldpc_source_hash(void) { return LDPC_STR(LDPC_SRC_HASH); }

// Host-side containers may throw; no exception crosses the C boundary.
#define LDPC_NOTHROW(call)                                                                     \
    try {                                                                                      \
        return call;                                                                           \
    } catch (const std::bad_alloc &) {                                                         \
        return fail(LDPC_ERR_HIP, "out of host memory");                                       \
    } catch (const std::exception &e) {                                                        \
        return fail(LDPC_ERR_HIP, "internal error: %s", e.what());                             \
    } catch (...) {                                                                            \
        return fail(LDPC_ERR_HIP, "internal error");                                           \
    }

// validates a CSR and fills the host copies of a graph
static int graph_host_build(HostGraph *g, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr, const int32_t *var_idx)
{
    if (n < 0 || m < 0 || E < 0 || !check_ptr || (E > 0 && !var_idx)) return fail(LDPC_ERR_ARG, "bad graph sizes");
    if (check_ptr[0] != 0 || check_ptr[m] != E) return fail(LDPC_ERR_ARG, "check_ptr must span [0, E]");
    for (int i = 0; i < m; ++i) {
        const int a = check_ptr[i], b = check_ptr[i + 1];
        if (b < a || b > E) return fail(LDPC_ERR_ARG, "check_ptr not monotone at check %d", i);
        for (int e = a; e < b; ++e) {
            const int j = var_idx[e];
            if (j < 0 || j >= n) return fail(LDPC_ERR_ARG, "var_idx[%d]=%d out of range", e, j);
            if (e > a && var_idx[e - 1] >= j) return fail(LDPC_ERR_ARG, "edges of check %d not strictly ascending", i);
        }
    }
    host_graph_fill(g, n, m, E, check_ptr, var_idx);
    return LDPC_OK;
}

static int graph_create_impl(ldpc_graph **out, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                             const int32_t *var_idx)
{
    if (!out) return fail(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    ldpc_graph *g = new (std::nothrow) ldpc_graph();
    if (!g) return fail(LDPC_ERR_ARG, "out of host memory");
    if (int rc = graph_host_build(g, n, m, E, check_ptr, var_idx)) {
        delete g;
        return rc;
    }
    const std::vector<int> &var_ptr = g->h_var_ptr, &csc = g->h_csc;
    if (hipGetDevice(&g->device) != hipSuccess) {
        delete g;
        return fail(LDPC_ERR_HIP, "no HIP device available");
    }
    int rc = upload(&g->check_ptr, check_ptr, (size_t)m + 1);
    if (!rc) rc = upload(&g->var_idx, var_idx, (size_t)E);
    if (!rc) rc = upload(&g->var_ptr, var_ptr.data(), (size_t)n + 1);
    if (!rc) rc = upload(&g->csc_edge, E > 0 ? csc.data() : nullptr, (size_t)E);
    std::vector<int> wide;
    for (int i = 0; i < m; ++i)
        if (check_ptr[i + 1] - check_ptr[i] > kWideCheck) wide.push_back(i);
    g->n_wide = (int)wide.size();
    if (!rc && g->n_wide) rc = upload(&g->wide_checks, wide.data(), wide.size());
    if (rc) {
        ldpc_graph_destroy(g);
        return rc;
    }
    *out = g;
    return LDPC_OK;
}

int ldpc_graph_create(ldpc_graph **out, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                      const int32_t *var_idx)
{
    LDPC_NOTHROW(graph_create_impl(out, n, m, E, check_ptr, var_idx))
}

static int graph_create_layered_impl(ldpc_graph **out, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                                     const int32_t *var_idx, int32_t n_layers, const int32_t *layer_ptr)
{
    if (!out) return fail(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    {
        HostGraph probe;                                             // validates the CSR before the partition reads it
        if (int rc = graph_host_build(&probe, n, m, E, check_ptr, var_idx)) return rc;
    }
    const std::string bad = layer_partition_error(n, m, check_ptr, var_idx, n_layers, layer_ptr);
    if (!bad.empty()) return fail(LDPC_ERR_ARG, "%s", bad.c_str());
    if (int rc = graph_create_impl(out, n, m, E, check_ptr, var_idx)) return rc;
    (*out)->h_layer_ptr.assign(layer_ptr, layer_ptr + n_layers + 1);
    return LDPC_OK;
}

int ldpc_graph_create_layered(ldpc_graph **out, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, int32_t n_layers, const int32_t *layer_ptr)
{
    LDPC_NOTHROW(graph_create_layered_impl(out, n, m, E, check_ptr, var_idx, n_layers, layer_ptr))
}

int ldpc_graph_layers(const ldpc_graph *g, int32_t *n_layers, int32_t *layer_ptr_out)
{
    if (!g || !n_layers) return fail(LDPC_ERR_ARG, "NULL argument");
    *n_layers = g->h_layer_ptr.empty() ? 0 : (int32_t)g->h_layer_ptr.size() - 1;
    if (layer_ptr_out && !g->h_layer_ptr.empty()) std::copy(g->h_layer_ptr.begin(), g->h_layer_ptr.end(), layer_ptr_out);
    return LDPC_OK;
}

void ldpc_graph_destroy(ldpc_graph *g)
{
    if (!g) return;
    DeviceGuard guard(g->device);
    (void)hipFree(g->check_ptr); (void)hipFree(g->var_idx); (void)hipFree(g->var_ptr); (void)hipFree(g->csc_edge);
    (void)hipFree(g->wide_checks);
    delete g;
}

int ldpc_graph_info(const ldpc_graph *g, int32_t out5[5])
{
    if (!g || !out5) return fail(LDPC_ERR_ARG, "NULL argument");
    out5[0] = g->n; out5[1] = g->m; out5[2] = g->E; out5[3] = g->max_dc; out5[4] = g->max_dv;
    return LDPC_OK;
}

static int decoder_create_impl(ldpc_decoder **out, const ldpc_graph *g, const ldpc_decoder_desc *desc)
{
    if (!out) return fail(LDPC_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!g || !desc) return fail(LDPC_ERR_ARG, "NULL argument");
    if (desc->dtype != LDPC_F32 && desc->dtype != LDPC_F64) return fail(LDPC_ERR_ARG, "bad dtype");
    if (desc->c2v_form < LDPC_C2V_NMS || desc->c2v_form > LDPC_C2V_SPA) return fail(LDPC_ERR_ARG, "bad c2v_form");
    if (desc->iters < 0) return fail(LDPC_ERR_ARG, "iters < 0");
    if (desc->n_beta_slots < 1 || desc->n_alpha_slots < 1 || !desc->beta || !desc->alpha ||
        (g->E > 0 && !desc->beta_slot) || (g->n > 0 && !desc->alpha_slot))
        return fail(LDPC_ERR_ARG, "weight tables missing");
    for (int e = 0; e < g->E; ++e)
        if (desc->beta_slot[e] < 0 || desc->beta_slot[e] >= desc->n_beta_slots) return fail(LDPC_ERR_ARG, "beta_slot[%d] out of range", e);
    for (int j = 0; j < g->n; ++j)
        if (desc->alpha_slot[j] < 0 || desc->alpha_slot[j] >= desc->n_alpha_slots) return fail(LDPC_ERR_ARG, "alpha_slot[%d] out of range", j);
    // association orders restated on the device: torch.sum below its cascade level, np.sum one block
    if (desc->dtype == LDPC_F32 && g->max_dv > 575) return fail(LDPC_ERR_UNSUPPORTED, "variable degree %d > 575 (fp32 sum order)", g->max_dv);
    if (desc->dtype == LDPC_F64 && g->max_dv > 128) return fail(LDPC_ERR_UNSUPPORTED, "variable degree %d > 128 (fp64 sum order)", g->max_dv);
    if (desc->schedule < LDPC_SCHED_FLOODING || desc->schedule > LDPC_SCHED_LAYERED) return fail(LDPC_ERR_ARG, "bad schedule");
    if (desc->c2v_form == LDPC_C2V_SPA) {
        if (desc->schedule != LDPC_SCHED_FLOODING)
            return fail(LDPC_ERR_UNSUPPORTED, "the sum-product form (LDPC_C2V_SPA) decodes under LDPC_SCHED_FLOODING only: layered "
                                              "belief propagation is not implemented");
        for (int i = 0; i < g->m; ++i)
            if (g->h_check_ptr[i + 1] - g->h_check_ptr[i] == 1)
                return fail(LDPC_ERR_UNSUPPORTED, "check %d has degree 1: its sum-product message is the empty product, an infinite "
                                                  "LLR (LDPC_C2V_SPA needs every check of degree 0 or >= 2)", i);
    }
    if (desc->schedule != LDPC_SCHED_FLOODING) {
        if (desc->dtype != LDPC_F32) return fail(LDPC_ERR_UNSUPPORTED, "layered schedule is fp32 only");
        if (desc->c2v_form != LDPC_C2V_RCQ && desc->schedule == LDPC_SCHED_LAYERED_REF)
            return fail(LDPC_ERR_UNSUPPORTED, "the reference's layered schedule exists for the RCQ decoder only (rcq_decoder.py:281-350); "
                                              "the min-sum forms take LDPC_SCHED_LAYERED");
        if (g->m == 1 && desc->schedule == LDPC_SCHED_LAYERED_REF)
            return fail(LDPC_ERR_UNSUPPORTED, "the reference's layered schedule on a single-check code");
    }
    if (desc->c2v_form == LDPC_C2V_RCQ) {
        if (desc->dtype != LDPC_F32) return fail(LDPC_ERR_UNSUPPORTED, "RCQ messages are fp32 only");
        if (desc->n_levels < 1 || desc->n_levels > 128) return fail(LDPC_ERR_UNSUPPORTED, "n_levels %d outside 1..128 (bc 1..8)", desc->n_levels);
        if (desc->n_quantizers < 1 || !desc->thresholds || (desc->iters > 0 && !desc->q_of_iter)) return fail(LDPC_ERR_ARG, "quantiser tables missing");
        for (int t = 0; t < desc->iters; ++t)
            if (desc->q_of_iter[t] < 0 || desc->q_of_iter[t] >= desc->n_quantizers) return fail(LDPC_ERR_ARG, "q_of_iter[%d] out of range", t);
    }
    if (desc->c2v_form == LDPC_C2V_OMS && desc->oms_alpha) {
        if (desc->n_oms_alpha_slots < 1 || (g->E > 0 && !desc->oms_alpha_slot)) return fail(LDPC_ERR_ARG, "oms_alpha tables missing");
        for (int e = 0; e < g->E; ++e)
            if (desc->oms_alpha_slot[e] < 0 || desc->oms_alpha_slot[e] >= desc->n_oms_alpha_slots) return fail(LDPC_ERR_ARG, "oms_alpha_slot[%d] out of range", e);
    }

    DeviceGuard guard(g->device);
    ldpc_decoder *d = new (std::nothrow) ldpc_decoder();
    if (!d) return fail(LDPC_ERR_ARG, "out of host memory");
    d->g = g; d->dtype = desc->dtype; d->form = desc->c2v_form; d->T = desc->iters; d->schedule = desc->schedule;
    d->n_beta = desc->n_beta_slots; d->n_alpha = desc->n_alpha_slots;
    const size_t es = d->elem();
    const size_t rows = (size_t)std::max(d->T, 1);
    int rc = LDPC_OK;
    auto up_bytes = [&](void **dst, const void *src, size_t bytes) {
        char *p = nullptr;
        int r = upload(&p, (const char *)src, bytes);
        *dst = p;
        return r;
    };
    // tables have max(T,1) rows on the device; with T == 0 row 0 is never read for arithmetic
    if (d->T > 0) {
        rc = up_bytes(&d->beta, desc->beta, rows * d->n_beta * es);
        if (!rc) rc = up_bytes(&d->alpha, desc->alpha, rows * d->n_alpha * es);
    } else {
        rc = up_bytes(&d->beta, nullptr, (size_t)d->n_beta * es);
        if (!rc) rc = up_bytes(&d->alpha, nullptr, (size_t)d->n_alpha * es);
    }
    if (!rc) rc = upload(&d->beta_slot, desc->beta_slot, (size_t)g->E);
    d->beta_per_check = true;
    for (int i = 0; i < g->m && d->beta_per_check; ++i)
        for (int e = g->h_check_ptr[i] + 1; e < g->h_check_ptr[i + 1]; ++e)
            if (desc->beta_slot[e] != desc->beta_slot[g->h_check_ptr[i]]) { d->beta_per_check = false; break; }
    if (!rc) rc = upload(&d->alpha_slot, desc->alpha_slot, (size_t)g->n);
    if (!rc && d->form == LDPC_C2V_RCQ) {
        d->n_levels = desc->n_levels; d->n_quant = desc->n_quantizers;
        d->q_of_iter.assign(desc->q_of_iter, desc->q_of_iter + d->T);
        if (d->q_of_iter.empty()) d->q_of_iter.push_back(0);
        const size_t L = d->n_levels, Q = d->n_quant;
        rc = upload(&d->thresholds, desc->thresholds, Q * L);
        fill_quantizer_lut(d, desc->thresholds);
        if (!rc) rc = upload(&d->lut, d->lut_host.data(), d->lut_host.size());
        if (!rc) rc = upload(&d->q_of_iter_dev, d->q_of_iter.data(), d->q_of_iter.size());
        std::vector<int> iota(L + 1);
        for (size_t k = 0; k <= L; ++k) iota[k] = (int)k;
        if (!rc) rc = upload(&d->level_iota, iota.data(), iota.size());
        if (!rc && Q * 2 * L * sizeof(float) > 64 * 1024) rc = fail(LDPC_ERR_UNSUPPORTED, "quantiser LUTs exceed 64 KiB of LDS");
    }
    if (!rc && d->form == LDPC_C2V_OMS && desc->oms_alpha && d->T > 0) {
        d->n_oms_alpha = desc->n_oms_alpha_slots;
        rc = up_bytes(&d->oms_alpha, desc->oms_alpha, rows * d->n_oms_alpha * es);
        if (!rc) rc = upload(&d->oms_alpha_slot, desc->oms_alpha_slot, (size_t)g->E);
    }
    // inverse slot maps of the gradient paths: the min-sum forms (ldpc_backward, ldpc_train_joint), RCQ (ldpc_train_joint_ste)
    // and the LDPC_SCHED_LAYERED decoders (ldpc_train_joint_layered: beta and the check-side alpha; ldpc_train_joint_layered_ste:
    // beta; the schedule has no variable-side alpha)
    const bool lay = d->schedule == LDPC_SCHED_LAYERED;
    if (!rc && d->dtype == LDPC_F32 && (d->schedule == LDPC_SCHED_FLOODING || lay)) {
        auto invert = [&](const int32_t *slot, int count, int n_slots, int **ptr_dev, int **items_dev) {
            std::vector<int> ptr((size_t)n_slots + 1, 0), items((size_t)std::max(count, 1), 0);
            for (int x = 0; x < count; ++x) ptr[slot[x] + 1]++;
            for (int k = 0; k < n_slots; ++k) ptr[k + 1] += ptr[k];
            std::vector<int> fill(ptr.begin(), ptr.end() - 1);
            for (int x = 0; x < count; ++x) items[fill[slot[x]]++] = x;         // ascending x inside a slot
            int r = upload(ptr_dev, ptr.data(), ptr.size());
            if (!r) r = upload(items_dev, items.data(), items.size());
            return r;
        };
        rc = invert(desc->beta_slot, g->E, d->n_beta, &d->beta_inv_ptr, &d->beta_inv_items);
        if (!rc && !lay) rc = invert(desc->alpha_slot, g->n, d->n_alpha, &d->alpha_inv_ptr, &d->alpha_inv_items);
        if (!rc && d->oms_alpha) rc = invert(desc->oms_alpha_slot, g->E, d->n_oms_alpha, &d->oms_inv_ptr, &d->oms_inv_items);
    }
    if (!rc && d->form == LDPC_C2V_RCQ && d->dtype == LDPC_F32 && d->schedule == LDPC_SCHED_FLOODING &&
        g->E > 0 && g->max_dv <= 8 && (long long)g->E * 256 < (1ll << 31) && (long long)g->n * 1024 < (1ll << 31)) {
        // gather metadata of the fused RCQ iteration (cn_gather): per CSR edge its variable, where the list of
        // the variable's OTHER edges starts (ascending check order = CSC order), how many there are, alpha column
        std::vector<int4> meta((size_t)g->E + 1);
        std::vector<int> nbr;
        nbr.reserve((size_t)g->E * 3 + 8);
        for (int e = 0; e < g->E; ++e) {
            const int j = g->h_var_idx[e], s0 = g->h_var_ptr[j], dv = g->h_var_ptr[j + 1] - s0;
            meta[e] = make_int4(j, (int)nbr.size(), dv - 1, desc->alpha_slot[j]);
            for (int k = 0; k < dv; ++k)
                if (g->h_csc[s0 + k] != e) nbr.push_back(g->h_csc[s0 + k]);
        }
        meta[g->E] = make_int4(0, 0, 0, 0);           // what the prefetch past the last edge of the last check reads
        nbr.resize(nbr.size() + 8, 0);
        rc = upload(&d->gat_meta, meta.data(), meta.size());
        if (!rc) rc = upload(&d->gat_nbr, nbr.data(), nbr.size());
        d->gat_ok = !rc;
    }
    if (!rc && d->form == LDPC_C2V_RCQ) apply_quantizer_flags(d, quantizer_flags(d, desc->thresholds));   // before the plans
    resident_table_flags(d, desc->alpha);
    beta_table_flags(d, desc->beta);
    // the sum-product form has the two-sweep streaming engine only: no LDS-resident plan is built for it
    if (!rc && d->schedule == LDPC_SCHED_FLOODING && d->form != LDPC_C2V_SPA) rc = build_resident_plan(d, desc);
    if (!rc) rc = build_layered_plan(d, desc);
    if (!rc) rc = build_block_plan(d, desc);
    if (rc) {
        ldpc_decoder_destroy(d);
        return rc;
    }
    *out = d;
    return LDPC_OK;
}

int ldpc_decoder_create(ldpc_decoder **out, const ldpc_graph *g, const ldpc_decoder_desc *desc)
{
    LDPC_NOTHROW(decoder_create_impl(out, g, desc))
}

int ldpc_decoder_set_mode(ldpc_decoder *d, int32_t mode)
{
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (mode < LDPC_MODE_AUTO || mode > LDPC_MODE_BLOCK) return fail(LDPC_ERR_ARG, "bad mode");
    if (mode == LDPC_MODE_BLOCK && !d->blk_ok)
        return fail(LDPC_ERR_UNSUPPORTED, "LDPC_MODE_BLOCK: %s", d->blk_why.c_str());
    if (d->form == LDPC_C2V_SPA && (mode == LDPC_MODE_RESIDENT || mode == LDPC_MODE_GATHER || mode == LDPC_MODE_PAIR))
        return fail(LDPC_ERR_UNSUPPORTED, "the sum-product form (LDPC_C2V_SPA) has the two-sweep streaming engine only "
                                          "(LDPC_MODE_AUTO / STREAM / SWEEPS): no LDS-resident, fused or code-pair form");
    if (mode == LDPC_MODE_GATHER && !d->gat_ok)
        return fail(LDPC_ERR_UNSUPPORTED, "the fused RCQ iteration needs an fp32 flooding RCQ decoder with variable degree <= 8");
    if (mode == LDPC_MODE_PAIR && !d->pair_ok)
        return fail(LDPC_ERR_UNSUPPORTED, "the code-pair form needs an fp32 flooding RCQ decoder with one beta per check, "
                                          "sorted thresholds and at most 62 levels");
    if (mode == LDPC_MODE_RESIDENT && !d->res_ok && !d->lay_ok)
        return fail(LDPC_ERR_UNSUPPORTED, "code does not qualify for the LDS-resident engine "
                                          "(dv <= 8, check degree <= 1024, state within 160 KiB of LDS)");
    d->mode = mode;
    return LDPC_OK;
}

int ldpc_decoder_info(const ldpc_decoder *d, int32_t out4[4])
{
    if (!d || !out4) return fail(LDPC_ERR_ARG, "NULL argument");
    out4[0] = (use_resident(d) || use_layered_lds(d)) ? LDPC_MODE_RESIDENT : use_pair(d) ? LDPC_MODE_PAIR : use_gather(d) ? LDPC_MODE_GATHER : LDPC_MODE_SWEEPS;
    out4[1] = d->res_ok ? (d->dtype == LDPC_F64 ? 1 : d->res_G) : 0;      // fp64: one codeword in a float pair's slots
    out4[2] = d->res_ok ? d->res_NT : 0;
    out4[3] = d->res_ok ? (int32_t)d->res_lds : 0;
    if (d->resc_ok) { out4[2] = kResCptThreads; out4[3] = (int32_t)d->resc_lds; }   // the fixed-T decode's compact geometry
    if (d->lay_ok) { out4[1] = d->lay.cw; out4[2] = kWave; out4[3] = (int32_t)d->lay_lds; }   // layered: codewords per (one-wave) workgroup
    if (use_block(d)) { out4[0] = LDPC_MODE_BLOCK; out4[1] = d->blk.G; out4[2] = d->blk_threads; out4[3] = (int32_t)d->blk_lds; }
    return LDPC_OK;
}

int ldpc_decoder_set_weights(ldpc_decoder *d, const void *beta, const void *alpha, const void *oms_alpha,
                             void *stream)
{
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (d->T == 0) return LDPC_OK;
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t es = d->elem(), rows = (size_t)d->T;
    if (beta) {
        HIP_TRY(hipMemcpyAsync(d->beta, beta, rows * d->n_beta * es, hipMemcpyHostToDevice, s));
        beta_table_flags(d, beta);
        if (int rc = gather_layered_beta(d, s)) return rc;
        if (int rc = gather_block_tables(d, true, false, s)) return rc;
    }
    if (alpha) {
        HIP_TRY(hipMemcpyAsync(d->alpha, alpha, rows * d->n_alpha * es, hipMemcpyHostToDevice, s));
        resident_table_flags(d, alpha);
    }
    if (oms_alpha) {
        if (!d->oms_alpha) return fail(LDPC_ERR_ARG, "decoder was created without oms_alpha");
        HIP_TRY(hipMemcpyAsync(d->oms_alpha, oms_alpha, rows * d->n_oms_alpha * es, hipMemcpyHostToDevice, s));
        if (int rc = gather_layered_oms(d, s)) return rc;
        if (int rc = gather_block_tables(d, false, true, s)) return rc;
    }
    return LDPC_OK;
}

static int set_quantizers_impl(ldpc_decoder *d, const float *thresholds, void *stream)
{
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (d->form != LDPC_C2V_RCQ) return fail(LDPC_ERR_UNSUPPORTED, "ldpc_decoder_set_quantizers: the decoder has no quantiser (LDPC_C2V_RCQ only)");
    if (!thresholds) return fail(LDPC_ERR_ARG, "NULL thresholds");
    const QuantizerFlags f = quantizer_flags(d, thresholds);
    // a forced form the new table does not admit: refuse before anything is touched (ldpc_decoder_set_mode's message)
    if (d->mode == LDPC_MODE_PAIR && !f.pair_ok)
        return fail(LDPC_ERR_UNSUPPORTED, "the code-pair form needs an fp32 flooding RCQ decoder with one beta per check, "
                                          "sorted thresholds and at most 62 levels");
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const size_t L = d->n_levels, Q = d->n_quant;
    HIP_TRY(hipMemcpyAsync(d->thresholds, thresholds, Q * L * sizeof(float), hipMemcpyHostToDevice, s));
    fill_quantizer_lut(d, thresholds);
    HIP_TRY(hipMemcpyAsync(d->lut, d->lut_host.data(), d->lut_host.size() * sizeof(float), hipMemcpyHostToDevice, s));
    apply_quantizer_flags(d, f);
    return LDPC_OK;
}

int ldpc_decoder_set_quantizers(ldpc_decoder *d, const float *thresholds, void *stream)
{
    LDPC_NOTHROW(set_quantizers_impl(d, thresholds, stream))
}

void ldpc_decoder_destroy(ldpc_decoder *d)
{
    if (!d) return;
    DeviceGuard guard(d->g->device);
    (void)hipFree(d->beta); (void)hipFree(d->alpha); (void)hipFree(d->oms_alpha);
    (void)hipFree(d->beta_slot); (void)hipFree(d->alpha_slot); (void)hipFree(d->oms_alpha_slot);
    (void)hipFree(d->thresholds); (void)hipFree(d->lut); (void)hipFree(d->q_of_iter_dev); (void)hipFree(d->level_iota);
    for (void *p : d->res_bufs) (void)hipFree(p);
    (void)hipFree(d->gat_meta); (void)hipFree(d->gat_nbr); (void)hipFree(d->lay_off);
    (void)hipFree(d->lay_slot); (void)hipFree(d->lay_beta); (void)hipFree(d->lay_oms_slot); (void)hipFree(d->lay_oms);
    (void)hipFree(d->blk_layer_ptr); (void)hipFree(d->blk_entry_base); (void)hipFree(d->blk_deg); (void)hipFree(d->blk_off);
    (void)hipFree(d->blk_slot); (void)hipFree(d->blk_beta); (void)hipFree(d->blk_oms_slot); (void)hipFree(d->blk_oms);
    (void)hipFree(d->beta_inv_ptr); (void)hipFree(d->beta_inv_items); (void)hipFree(d->alpha_inv_ptr);
    (void)hipFree(d->alpha_inv_items); (void)hipFree(d->oms_inv_ptr); (void)hipFree(d->oms_inv_items);
    delete d;
}

size_t ldpc_decoder_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    if (!d || batch < 0) return 0;
    if (use_resident(d) || use_layered_lds(d) || use_block(d)) return kAlign;   // the LDS-resident engines keep their state in LDS
    return carve(d, batch, nullptr).total;
}

int ldpc_decode(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t *bits,
                void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed_bits,
                void *workspace, size_t workspace_bytes, void *stream)
{
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch == 0) return LDPC_OK;
    if (!llr || !workspace) return fail(LDPC_ERR_ARG, "NULL llr/workspace");
    if (d->g->n == 0) return LDPC_OK;
    if (((uintptr_t)workspace % kAlign) != 0) return fail(LDPC_ERR_ARG, "workspace must be %zu-byte aligned", kAlign);
    if (use_resident(d))
        return decode_resident(d, llr, batch, early_stop, bits, posterior, iterations, success, packed_bits, nullptr, stream);
    if (use_block(d))
        return decode_block(d, llr, batch, early_stop, bits, posterior, iterations, success, packed_bits, stream);
    if (use_layered_lds(d))
        return decode_layered_lds(d, llr, batch, early_stop, bits, posterior, iterations, success, packed_bits, stream);
    const Workspace w = carve(d, batch, workspace);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    if ((size_t)w.tiles * ((d->g->n + 3) / 4) > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    if (d->dtype == LDPC_F64)
        return decode_dispatch<double>(d, llr, batch, early_stop != 0, bits, posterior, iterations, success, packed_bits, w, s);
    return decode_dispatch<float>(d, llr, batch, early_stop != 0, bits, posterior, iterations, success, packed_bits, w, s);
}

int ldpc_decode_capped(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t max_iterations,
                       int32_t *bits, void *posterior, int32_t *iterations, uint8_t *success, uint8_t *packed_bits,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (max_iterations < 1) return fail(LDPC_ERR_ARG, "max_iterations must be >= 1");
    IterCap cap(max_iterations);
    return ldpc_decode(d, llr, batch, early_stop, bits, posterior, iterations, success, packed_bits, workspace, workspace_bytes,
                       stream);
}

}  // extern "C"

// ---- gradient (training) path: ldpc_train_host.hip over the kernels of ldpc_train.hip --------------------------
#include "ldpc_train_host.hip"

// ---- on-device Monte-Carlo: AWGN channel, error counters, one SNR point (ldpc_channel_awgn / ldpc_sim_count / ldpc_simulate)
#include "ldpc_sim.hip"

// ---- random codewords: device encoder, per-frame channel, one SNR point on them (ldpc_encode* / ldpc_channel_awgn_cw / ldpc_simulate_enc)
#include "ldpc_encode.hip"

// ---- symbol channel: Gray-mapped QAM, Rayleigh fading, max-log demapper, one SNR point on it (ldpc_channel_sym / ldpc_simulate_sym)
#include "ldpc_modulation.hip"

// ---- constellation channel: a table of up to 64 labelled points, joint max-log / exact demapper (ldpc_channel_con / ldpc_demap_con / ldpc_simulate_con)
#include "ldpc_constellation.hip"

extern "C" {

int ldpc_debug_key4(const float *values, int64_t count, float beta, const float thresholds4[4], uint8_t *keys_float,
                    uint8_t *keys_compare, void *stream)
{
    if (!values || !thresholds4 || !keys_float || !keys_compare || count <= 0) return fail(LDPC_ERR_ARG, "bad argument");
    const long long pairs = (count + 1) / 2;
    hipLaunchKernelGGL(debug_key4, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values,
                       (long long)count, beta, thresholds4, keys_float, keys_compare);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int ldpc_debug_min2(const float *values, int64_t rows, int32_t d, float *m12_chain, uint32_t *par_chain, float *m12_pair,
                    uint32_t *par_pair, void *stream)
{
    if (!values || !m12_chain || !par_chain || !m12_pair || !par_pair || rows <= 0 || d < 1 || d > 32)
        return fail(LDPC_ERR_ARG, "bad argument");
    const long long threads = (rows + 1) / 2;
    if ((threads + 255) / 256 > 0x7fffffffll) return fail(LDPC_ERR_ARG, "too many rows for one launch");
    hipLaunchKernelGGL(debug_min2, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)stream, values,
                       (long long)rows, (int)d, m12_chain, par_chain, m12_pair, par_pair);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

int ldpc_debug_workspace_layout(const ldpc_decoder *d, int64_t batch, int32_t max_iterations, int64_t out8[8])
{
    if (!d || !out8 || batch <= 0) return fail(LDPC_ERR_ARG, "bad argument");
    if (use_resident(d) || use_layered_lds(d) || use_block(d)) return fail(LDPC_ERR_ARG, "workspace layout exists only in LDPC_MODE_STREAM");
    char *base = reinterpret_cast<char *>(kAlign);   // any non-null base: only differences are used
    const Workspace w = carve(d, batch, base);
    out8[0] = w.vec; out8[1] = w.tiles;
    // fused RCQ form: the codes ping-pong between the two buffers, the last iteration it leaves them in buffer it & 1
    const int T_run = max_iterations > 0 ? std::min(d->T, (int)max_iterations) : d->T;
    const char *c2v_final = (use_gather(d) && T_run > 0 && ((T_run - 1) & 1)) ? w.v2c : w.c2v;
    out8[2] = w.llrT - base; out8[3] = w.v2c - base; out8[4] = c2v_final - base; out8[5] = w.postT - base;
    out8[6] = (char *)w.bitsT - base; out8[7] = (char *)w.done - base;
    return LDPC_OK;
}

// The compact plan a debug hook reports: a decoder's stored layout, or (d == NULL) a layout planned from these arrays on
// host copies only -- no device is touched.  `place` = false stops before the placement search (cpt_layout), for a
// hook that needs the check order alone.
struct CompactView {
    HostGraph own_g;
    CptLayout own;
    const HostGraph *g = &own_g;
    const CptLayout *L = &own;
    std::vector<ResVCheck> vc;                           // the degree-sorted checks (resident_checks)
    long long Sc = 0;
};

static int compact_view(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                        const int32_t *var_idx, bool place, CompactView &v)
{
    if (d) {
        if (!d->resc_ok) return fail(LDPC_ERR_UNSUPPORTED, "the decoder has no compact fixed-T plan");
        v.L = &d->resc_layout; v.g = d->g; v.Sc = d->resc.S;
    } else if (int rc = graph_host_build(&v.own_g, n, m, E, check_ptr, var_idx)) {
        return rc;
    }
    if (!resident_checks(v.g, v.vc) || (!d && !cpt_geometry(v.g, v.vc, v.Sc)))
        return fail(LDPC_ERR_UNSUPPORTED, "the graph does not qualify for the compact plan");
    if (!d && place) cpt_layout(v.g, v.vc, v.Sc, v.own);
    return LDPC_OK;
}

static int compact_layout_impl(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                               const int32_t *var_idx, int32_t *pos_of_var, uint8_t *cells, int32_t *stats)
{
    CompactView v;
    if (int rc = compact_view(d, n, m, E, check_ptr, var_idx, true, v)) return rc;
    const CptLayout *L = v.L;
    if (pos_of_var) {
        for (int j = 0; j < v.g->n; ++j) pos_of_var[j] = -1;
        for (int q = 0; q < (int)L->var_at.size(); ++q)
            if (L->var_at[q] >= 0) pos_of_var[L->var_at[q]] = q;
    }
    if (cells)
        for (int c = 0; c < kCptCells; ++c) cells[c] = (uint8_t)(L->cell[c / kResRegVars] >> (8 * (c % kResRegVars)));
    if (stats) {
        stats[0] = (int32_t)L->var_at.size(); stats[1] = L->worst; stats[2] = L->total; stats[3] = L->mixed;
    }
    return LDPC_OK;
}

int ldpc_debug_compact_layout(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, int32_t *pos_of_var, uint8_t cells[32], int32_t stats[4])
{
    LDPC_NOTHROW(compact_layout_impl(d, n, m, E, check_ptr, var_idx, pos_of_var, cells, stats))
}

static int compact_checks_impl(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                               const int32_t *var_idx, uint32_t *words)
{
    if (!words) return fail(LDPC_ERR_ARG, "NULL argument");
    CompactView v;
    if (int rc = compact_view(d, n, m, E, check_ptr, var_idx, false, v)) return rc;
    unsigned own[kCptWaves];
    if (!d) cpt_check_words(v.vc, true, own);
    const unsigned *src = d ? d->resc.ccell : own;
    std::copy(src, src + kCptWaves, words);
    return LDPC_OK;
}

int ldpc_debug_compact_checks(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, uint32_t words[8])
{
    LDPC_NOTHROW(compact_checks_impl(d, n, m, E, check_ptr, var_idx, words))
}

static int compact_banks_impl(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                              const int32_t *var_idx, int32_t *slot_of_edge, int32_t *pos_of_check, int32_t *model,
                              int32_t *base_slot_of_edge, int32_t *base_pos_of_check, int32_t *base_model,
                              int32_t *geometry)
{
    CompactView v;
    if (int rc = compact_view(d, n, m, E, check_ptr, var_idx, true, v)) return rc;
    const CptLayout *L = v.L;
    auto emit = [&](const std::vector<int> &slots, const std::vector<int> &check_at, const int (&banks)[4],
                    int32_t *slots_out, int32_t *pos_out, int32_t *model_out) {
        if (slots_out) std::copy(slots.begin(), slots.end(), slots_out);
        if (pos_out)
            for (int p = 0; p < (int)check_at.size(); ++p) pos_out[v.vc[check_at[p]].check] = p;
        if (model_out) std::copy(banks, banks + 4, model_out);
    };
    emit(L->slot_of_edge, L->check_at, L->banks, slot_of_edge, pos_of_check, model);
    emit(L->base_slot_of_edge, L->base_check_at, L->base_banks, base_slot_of_edge, base_pos_of_check, base_model);
    if (geometry) { geometry[0] = kResCptStride; geometry[1] = (int32_t)v.Sc; }
    return LDPC_OK;
}

int ldpc_debug_compact_banks(const ldpc_decoder *d, int32_t n, int32_t m, int32_t E, const int32_t *check_ptr,
                             const int32_t *var_idx, int32_t *slot_of_edge, int32_t *pos_of_check, int32_t model[4],
                             int32_t *base_slot_of_edge, int32_t *base_pos_of_check, int32_t base_model[4],
                             int32_t geometry[2])
{
    LDPC_NOTHROW(compact_banks_impl(d, n, m, E, check_ptr, var_idx, slot_of_edge, pos_of_check, model, base_slot_of_edge,
                                    base_pos_of_check, base_model, geometry))
}
int ldpc_debug_resident_kernel(const ldpc_decoder *d, int32_t early_stop, int32_t out12[12])
{
    if (!d || !out12) return fail(LDPC_ERR_ARG, "NULL argument");
    if (d->schedule != LDPC_SCHED_FLOODING || !use_resident(d))       // the layered schedules never launch resident_decode
        return fail(LDPC_ERR_UNSUPPORTED, "the decoder does not decode with resident_decode (flooding schedule on the LDS-resident engine)");
    const ResidentKernel k = resident_kernel(d, early_stop != 0);
    const ResidentPlan &pl = k.plan == kResPlanCompact ? d->resc : d->res;
    const int32_t out[12] = {k.plan, k.G, k.form == FORM_NMS ? LDPC_C2V_NMS : k.form == FORM_OMS ? LDPC_C2V_OMS : LDPC_C2V_RCQ,
                             k.bpc, k.nl, k.ms, pl.mstride, k.split, d->unit_alpha, d->rcq_zero0,
                             d->form == LDPC_C2V_OMS && d->oms_alpha != nullptr, k.alpha_in_lds};
    std::copy(out, out + 12, out12);
    return LDPC_OK;
}

int ldpc_debug_boundary_kernels(const ldpc_decoder *d, int64_t batch, int32_t max_iterations, int32_t saving,
                                const void *llr, const void *posterior, const int32_t *bits, int32_t out5[5])
{
    if (!d || !out5) return fail(LDPC_ERR_ARG, "NULL argument");
    if (batch <= 0) return fail(LDPC_ERR_ARG, "batch must be >= 1");
    if (saving) {
        if (int rc = train_supported(d)) return rc;                   // ldpc_decode_saving streams whatever the mode
    } else if (use_resident(d) || use_layered_lds(d) || use_block(d))
        return fail(LDPC_ERR_UNSUPPORTED, "the LDS-resident kernels read and write the caller's rows element by element");
    IterCap cap(max_iterations > 0 ? max_iterations : INT_MAX);      // as ldpc_decode_capped; <= 0: the decoder's T
    const BoundaryKernels k = boundary_kernels(d, pick_vec(d, batch), capped_T(d), saving != 0, llr, posterior, bits);
    const int32_t out[5] = {k.vec, k.in_bytes, k.fused_in, k.out_path, k.out_bytes};
    std::copy(out, out + 5, out5);
    return LDPC_OK;
}

static int debug_layer_plan_impl(int32_t n, int32_t m, int32_t E, const int32_t *check_ptr, const int32_t *var_idx,
                                 int32_t n_layers, const int32_t *layer_ptr, int32_t kind, int64_t out8[8])
{
    if (!out8) return fail(LDPC_ERR_ARG, "NULL argument");
    if (kind != kBlkMinSum && kind != kBlkRcq) return fail(LDPC_ERR_ARG, "kind must be 0 (min-sum) or 1 (RCQ)");
    HostGraph probe;
    if (int rc = graph_host_build(&probe, n, m, E, check_ptr, var_idx)) return rc;
    const std::string bad = layer_partition_error(n, m, check_ptr, var_idx, n_layers, layer_ptr);
    if (!bad.empty()) return fail(LDPC_ERR_ARG, "%s", bad.c_str());
    const LayerPlan p = layer_plan(n, m, check_ptr, var_idx, n_layers, layer_ptr, kind);
    std::fill(out8, out8 + 8, (int64_t)0);
    if (!p.ok) { (void)fail(LDPC_OK, "%s", p.why.c_str()); return LDPC_OK; }
    const int64_t out[8] = {1, p.G, p.lpc, p.threads, (int64_t)p.lds_bytes, (int64_t)p.row_words, p.entries, p.W};
    std::copy(out, out + 8, out8);
    return LDPC_OK;
}

int ldpc_debug_layer_plan(int32_t n, int32_t m, int32_t E, const int32_t *check_ptr, const int32_t *var_idx,
                          int32_t n_layers, const int32_t *layer_ptr, int32_t kind, int64_t out8[8])
{
    LDPC_NOTHROW(debug_layer_plan_impl(n, m, E, check_ptr, var_idx, n_layers, layer_ptr, kind, out8))
}

int ldpc_debug_launch_geometry(const ldpc_decoder *d, int64_t batch, int64_t out8[8])
{
    if (!d || !out8) return fail(LDPC_ERR_ARG, "NULL argument");
    if (batch <= 0) return fail(LDPC_ERR_ARG, "batch must be >= 1");
    if (use_resident(d) || use_layered_lds(d) || use_block(d))
        return fail(LDPC_ERR_UNSUPPORTED, "the LDS-resident kernels have no tiles: launch geometry exists only on the streaming engine");
    const Workspace w = carve(d, batch, nullptr);
    const bool flooding = d->schedule == LDPC_SCHED_FLOODING;      // the layered kernels check the syndrome themselves
    const bool gather = flooding && d->dtype == LDPC_F32 && use_gather(d);
    const GatherTiles gt = gather ? gather_tiles(d->g->n, d->g->E, w.tiles, 64 * w.vec) : GatherTiles{0, (size_t)w.tiles};
    const int64_t out[8] = {w.vec, w.tiles, flooding ? syndrome_chunks(d->g->m, w.tiles) : 0, gt.xcd_tiles, (int64_t)gt.padded, 0, 0, 0};
    std::copy(out, out + 8, out8);
    return LDPC_OK;
}

int ldpc_debug_resident_c2v(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop,
                            int32_t max_iterations, void *posterior, int32_t *iterations, void *c2v_out, void *stream)
{
    if (!d || !llr || !posterior || !c2v_out || batch <= 0) return fail(LDPC_ERR_ARG, "bad argument");
    if (!use_resident(d)) return fail(LDPC_ERR_ARG, "the decoder is not on the LDS-resident engine");
    if (d->g->n == 0) return LDPC_OK;
    IterCap cap(max_iterations > 0 ? max_iterations : INT_MAX);      // as ldpc_decode_capped; <= 0: the decoder's T
    return decode_resident(d, llr, batch, early_stop, nullptr, posterior, iterations, nullptr, nullptr, c2v_out, stream);
}

int ldpc_debug_sweep(const ldpc_decoder *d, int64_t batch, int32_t which, int32_t iter, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    if (!d || !workspace || batch <= 0) return fail(LDPC_ERR_ARG, "bad argument");
    if (iter < 0 || iter >= d->T) return fail(LDPC_ERR_ARG, "iter outside [0, T)");
    if (use_resident(d) || use_layered_lds(d) || use_block(d)) return fail(LDPC_ERR_ARG, "debug sweeps need LDPC_MODE_STREAM");
    const Workspace w = carve(d, batch, workspace);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace too small");
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    const bool f64 = d->dtype == LDPC_F64;
    if (use_pair(d) && !f64) {
        // code-pair form: which = 0 the check sweep (integer-only from iteration 1), which = 1 the variable sweep
        // (code-producing except in the last iteration)
        if (which == 0 && (iter >= 1 || (w.vec == 4 && pair_q4<4>(d))))
            return w.vec == 1 ? launch_cn_q<1>(d, w, iter, false, s) : launch_cn_q<4>(d, w, iter, false, s);
        if (which != 0 && iter < d->T - 1) return w.vec == 1 ? launch_vn_q<1>(d, w, iter, false, s) : launch_vn_q<4>(d, w, iter, false, s);
    }
    if (use_gather(d) && !f64) {
        // fused RCQ form: which = 0 is the fused iteration kernel (iter >= 1; iteration 0 is the plain check sweep),
        // which = 1 the posterior-only variable pass
        char *buf[2] = {w.c2v, w.v2c};
        if (which == 0 && iter >= 1)
            return w.vec == 1 ? launch_gather<1>(d, w, iter, false, buf[(iter - 1) & 1], buf[iter & 1], s)
                              : launch_gather<4>(d, w, iter, false, buf[(iter - 1) & 1], buf[iter & 1], s);
        if (which != 0) {
            Workspace wv = w;
            wv.c2v = buf[iter & 1];
            return w.vec == 1 ? launch_vn<float, 1>(d, wv, iter, true, false, s) : launch_vn<float, 4>(d, wv, iter, true, false, s);
        }
    }
#define LDPC_DBG(REAL_, V_)                                                                 \
    return which == 0 ? launch_cn<REAL_, V_>(d, w, iter, false, s)                           \
                      : launch_vn<REAL_, V_>(d, w, iter, iter == d->T - 1, false, s)
    if (f64) {
        if (w.vec == 1) { LDPC_DBG(double, 1); } else { LDPC_DBG(double, 2); }
    } else {
        if (w.vec == 1) { LDPC_DBG(float, 1); } else { LDPC_DBG(float, 4); }
    }
#undef LDPC_DBG
}

}  // extern "C"
