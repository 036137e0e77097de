// ldpc_train_host.hip -- host side of the gradient (training) path over the kernels in ldpc_train.hip: the saving decode and
// its backward sweeps (ldpc_decode_saving / ldpc_backward), and posterior joint training (ldpc_train_joint,
// ldpc_train_joint_ste, ldpc_train_joint_layered, ldpc_train_joint_layered_ste: one workspace carver and one loop for the four,
// and for the two ..._levels forms of the quantised ones, which add the level gradient of the learned quantisers).
//
// Not a unit of its own: ldpc_hip.hip includes it after the decode entry points and it uses that file's Workspace, carve,
// pick_vec, launch_cn, launch_vn, decode_dispatch, saved_layout, fail, HIP_TRY and DeviceGuard.
#include <type_traits>

namespace {
// the sum-product form is a decode-only baseline: every gradient entry point refuses it with this message
int spa_no_gradient()
{
    return fail(LDPC_ERR_UNSUPPORTED, "the sum-product form (LDPC_C2V_SPA) has no gradient path: ldpc_decode_saving, ldpc_backward "
                                      "and the ldpc_train_joint* entry points exist for the min-sum and RCQ forms");
}

int train_supported(const ldpc_decoder *d)
{
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (d->form == LDPC_C2V_SPA) return spa_no_gradient();
    if (d->schedule != LDPC_SCHED_FLOODING && d->form != LDPC_C2V_RCQ)
        return fail(LDPC_ERR_UNSUPPORTED, "the layered schedule (LDPC_SCHED_LAYERED) has no gradient path: gradients exist for "
                                          "the fp32 normalised / offset min-sum decoders under LDPC_SCHED_FLOODING");
    if (d->dtype != LDPC_F32 || d->form == LDPC_C2V_RCQ || d->schedule != LDPC_SCHED_FLOODING)
        return fail(LDPC_ERR_UNSUPPORTED, "gradients exist for the fp32 normalised / offset min-sum flooding decoders "
                                          "(the reference's RCQ quantiser passes no gradient)");
    return LDPC_OK;
}

struct BackwardWs {
    int vec = 0, tiles = 0;
    float *llrT = nullptr, *gpostT = nullptr, *gv2c = nullptr, *gc2v = nullptr, *gbeta = nullptr, *galpha = nullptr;
    float *goa = nullptr;             // offset form: per-edge partials of the check-side alpha
    float *gllrT = nullptr;           // accumulator of d loss/d llr (starts as a copy of gpostT)
    size_t part_bytes = 0, total = 0;
};
BackwardWs carve_backward(const ldpc_decoder *d, int64_t batch, void *base)
{
    BackwardWs w;
    w.vec = pick_vec(d, batch);
    const int W = 64 * w.vec;
    w.tiles = (int)std::max<int64_t>((batch + W - 1) / W, 1);
    const size_t n = d->g->n, E = std::max(d->g->E, 1), tw = (size_t)w.tiles * W, T = std::max(d->T, 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
    const size_t o_llr = take(tw * n * 4), o_gp = take(tw * n * 4), o_gv = take(tw * E * 4), o_gc = take(tw * E * 4);
    const size_t o_gb = take(T * w.tiles * E * 4), o_ga = take(T * w.tiles * n * 4);
    const size_t o_goa = take(d->form == LDPC_C2V_OMS ? T * w.tiles * E * 4 : 0);
    w.part_bytes = off - o_gb;
    const size_t o_gl = take(tw * n * 4);
    w.total = off;
    if (base) {
        char *b = (char *)base;
        w.llrT = (float *)(b + o_llr); w.gpostT = (float *)(b + o_gp); w.gv2c = (float *)(b + o_gv);
        w.gc2v = (float *)(b + o_gc); w.gbeta = (float *)(b + o_gb); w.galpha = (float *)(b + o_ga);
        w.goa = (float *)(b + o_goa);
        w.gllrT = (float *)(b + o_gl);
    }
    return w;
}

template <int VEC>
int backward_impl(const ldpc_decoder *d, const char *saved, const float *llr, int64_t batch, const int32_t *iterations,
                  const float *grad_posterior, float *grad_beta, float *grad_alpha, float *grad_oms_alpha,
                  float *grad_llr, const BackwardWs &w, hipStream_t s)
{
    constexpr int W = 64 * VEC;
    constexpr int JT = transpose_vars<float>();
    const GraphDev g = d->g->dev();
    const int T = d->T, vc = (g.n + JT - 1) / JT;
    const SavedLayout sl = saved_layout(d, w.tiles, W);
    const dim3 tgrid((unsigned)((size_t)w.tiles * VEC * vc)), blk(kBlock);
    hipLaunchKernelGGL((transpose_in<float, VEC>), tgrid, blk, 0, s, llr, w.llrT, (long long)batch, g.n, vc);
    hipLaunchKernelGGL((transpose_in<float, VEC>), tgrid, blk, 0, s, grad_posterior, w.gpostT, (long long)batch, g.n, vc);
    HIP_TRY(hipMemsetAsync(w.gbeta, 0, w.part_bytes, s));
    if (grad_llr)
        HIP_TRY(hipMemcpyAsync(w.gllrT, w.gpostT, (size_t)w.tiles * W * g.n * sizeof(float), hipMemcpyDeviceToDevice, s));
    const int cb = (g.m + kWavesPerBlock - 1) / kWavesPerBlock, vb = (g.n + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vbb = (g.n + kWavesPerBlock * kVnbVarsPerWave - 1) / (kWavesPerBlock * kVnbVarsPerWave);   // vn_backward: several variables per wave
    const dim3 cgrid((unsigned)((size_t)w.tiles * cb)), vgrid((unsigned)((size_t)w.tiles * vb)), vbgrid((unsigned)((size_t)w.tiles * vbb));
    const size_t epart = (size_t)w.tiles * g.E, vpart = (size_t)w.tiles * g.n;
    for (int t = T - 1; t >= 0; --t) {
        const float *beta_row = (const float *)d->beta + (size_t)t * d->n_beta;
        // d loss/d c2v_t is in w.gc2v (written by the variable pass of step t+1; unread at t == T-1)
        const bool oms = d->form == LDPC_C2V_OMS;
        float *goa = (oms && d->oms_alpha) ? w.goa + (size_t)t * epart : nullptr;
#define LDPC_CNB(FIRST_, FORM_, SRC_, OUT_)                                                                            \
    hipLaunchKernelGGL((cn_backward<VEC, FIRST_, FORM_>), cgrid, blk, 0, s, g, (const float *)(SRC_),                  \
                       (const float *)w.gc2v, (const float *)w.gpostT, iterations, (long long)batch, t, beta_row,     \
                       (const int *)d->beta_slot, (float *)(OUT_), w.gbeta + (size_t)t * epart, goa, cb)
        float *gv0 = grad_llr ? w.gv2c : nullptr;        // d loss/d v2c_0 is needed only for the input gradient
        if (t == 0) {
            if (oms) LDPC_CNB(true, FORM_OMS, w.llrT, gv0); else LDPC_CNB(true, FORM_NMS, w.llrT, gv0);
        } else {
            if (oms) LDPC_CNB(false, FORM_OMS, saved + sl.v2c_off(t), w.gv2c);
            else LDPC_CNB(false, FORM_NMS, saved + sl.v2c_off(t), w.gv2c);
            const float *alpha_row = (const float *)d->alpha + (size_t)(t - 1) * d->n_alpha;
            hipLaunchKernelGGL((vn_backward<VEC>), vbgrid, blk, 0, s, g, (const float *)(saved + sl.c2v_off(t - 1)),
                               (const float *)w.gv2c, iterations, (long long)batch, t, alpha_row, (const int *)d->alpha_slot,
                               w.gc2v, w.galpha + (size_t)(t - 1) * vpart, vbb);
        }
        if (grad_llr)                                     // g_llr += sum over the edges of every variable of g_v2c_t
            hipLaunchKernelGGL((llr_backward_accumulate<VEC>), vgrid, blk, 0, s, g, (const float *)w.gv2c, w.gllrT, vb);
#undef LDPC_CNB
    }
    HIP_TRY(hipGetLastError());
    if (grad_llr)
        hipLaunchKernelGGL((transpose_out<float, VEC>), tgrid, blk, 0, s, (const float *)w.gllrT, (const uint64_t *)nullptr, grad_llr,
                           (int *)nullptr, (long long)batch, g.n, vc);     // [tile][n][W] -> [batch][n], padding rows dropped
    // fixed-order reductions (one wave per slot and iteration): every table entry is written, no memset, no atomics
    if (grad_beta)
        hipLaunchKernelGGL(reduce_table_grads<float>, dim3((unsigned)d->n_beta, (unsigned)T), dim3(kWave), 0, s,
                           (const float *)w.gbeta, w.tiles, g.E, (const int *)d->beta_inv_ptr,
                           (const int *)d->beta_inv_items, d->n_beta, grad_beta);
    if (grad_oms_alpha && d->form == LDPC_C2V_OMS && d->oms_alpha)
        hipLaunchKernelGGL(reduce_table_grads<float>, dim3((unsigned)d->n_oms_alpha, (unsigned)T), dim3(kWave), 0, s,
                           (const float *)w.goa, w.tiles, g.E, (const int *)d->oms_inv_ptr,
                           (const int *)d->oms_inv_items, d->n_oms_alpha, grad_oms_alpha);
    if (grad_alpha)
        hipLaunchKernelGGL(reduce_table_grads<float>, dim3((unsigned)d->n_alpha, (unsigned)T), dim3(kWave), 0, s,
                           (const float *)w.galpha, w.tiles, g.n, (const int *)d->alpha_inv_ptr,
                           (const int *)d->alpha_inv_items, d->n_alpha, grad_alpha);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

// ---- posterior joint training (ldpc_train_joint, ldpc_train_joint_ste, ldpc_train_joint_layered, ldpc_train_joint_layered_ste) ----
// The fixed-T decode with the loss of every iteration's posterior and its posterior-local gradient formed while that
// iteration is decoded: nothing of earlier iterations is kept, so the scratch is a constant number of rows per codeword
// whatever T is.  One loop (joint_impl) for the four entry points; the entry point passes the kind:
//   kJointMinsum   flooding NMS / OMS.  E rows: v2c_t / v2c_t+1 and c2v_t-1 / c2v_t (ping-pong; the alpha_t-1 partial reads the
//                  leave-one-out sums of c2v_t-1), d J/d v2c_t;  n rows: llr, posterior (then g_l in place), targets, d J/d llr.
//   kJointSte      flooding RCQ (`codes`): the same on the two-sweep RCQ form -- the two C2V buffers hold 1-byte codes.
//   kJointLayered  layered NMS / OMS: layered_minsum_iter walks the checks once per launch on the running posteriors and keeps
//                  u_e = P_v - R_e of every edge; J_t and its seed g_l are formed on a COPY of the posterior rows (the walk
//                  still needs P), and cn_backward<..., LOCAL> differentiates the check update with v2c_t := u.  E rows: R, U,
//                  d J/d u;  n rows: posterior, its copy (then g_l), targets, d J/d llr.  Layered decoders run at VEC = 1.
//   kJointLayeredSte  layered RCQ (LDPC_SCHED_LAYERED): layered_rcq_iter is the walk, the messages it keeps are 1-byte codes
//                  (one row set: iteration t reads and rewrites the code of every edge), and cn_backward<..., FORM_RCQ, LOCAL>
//                  differentiates the check update with v2c_t := u and the straight-through mask read from the codes the walk
//                  just wrote.  E rows: U and d J/d u in fp32, the codes as bytes;  n rows as kJointLayered.
// Every kind adds per-tile partials of the table gradients and of the loss.  The ..._levels entry points of the two quantised
// kinds add, behind everything else, the partials of level_grad (d J_t / d the reconstruction value of every level).
enum { kJointMinsum = 0, kJointSte = 1, kJointLayered = 2, kJointLayeredSte = 3 };

int joint_supported(const ldpc_decoder *d, int kind)
{
    if (kind == kJointMinsum) return train_supported(d);
    if (!d) return fail(LDPC_ERR_ARG, "NULL decoder");
    if (d->form == LDPC_C2V_SPA) return spa_no_gradient();
    if (kind == kJointSte) {    // the quantised decoder, differentiated with the straight-through rule
        if (d->dtype != LDPC_F32 || d->form != LDPC_C2V_RCQ || d->schedule != LDPC_SCHED_FLOODING)
            return fail(LDPC_ERR_UNSUPPORTED, "the straight-through joint loss exists for the fp32 RCQ flooding decoders "
                                              "(ldpc_train_joint has the min-sum forms; the RCQ decoder under LDPC_SCHED_LAYERED takes "
                                              "ldpc_train_joint_layered_ste, the reference's layered schedule has no gradient path)");
        return LDPC_OK;
    }
    if (kind == kJointLayeredSte) {     // the quantised decoder on the paper's layered schedule
        if (d->dtype != LDPC_F32)
            return fail(LDPC_ERR_UNSUPPORTED, "the layered straight-through joint loss exists for fp32 decoders only (a float64 "
                                              "decoder has no layered schedule and no RCQ form)");
        if (d->schedule == LDPC_SCHED_FLOODING && d->form == LDPC_C2V_RCQ)
            return fail(LDPC_ERR_UNSUPPORTED, "a flooding RCQ decoder takes ldpc_train_joint_ste, not ldpc_train_joint_layered_ste");
        if (d->schedule == LDPC_SCHED_FLOODING)
            return fail(LDPC_ERR_UNSUPPORTED, "a flooding min-sum decoder takes ldpc_train_joint, not ldpc_train_joint_layered_ste");
        if (d->form != LDPC_C2V_RCQ)
            return fail(LDPC_ERR_UNSUPPORTED, "a layered min-sum decoder takes ldpc_train_joint_layered, not ldpc_train_joint_layered_ste");
        if (d->schedule != LDPC_SCHED_LAYERED)
            return fail(LDPC_ERR_UNSUPPORTED, "the layered straight-through joint loss exists for the RCQ decoder under "
                                              "LDPC_SCHED_LAYERED; the reference's layered schedule (LDPC_SCHED_LAYERED_REF) has no "
                                              "gradient path");
        return LDPC_OK;
    }
    // kJointLayered: the fp32 layered normalised / offset min-sum decoders
    if (d->dtype != LDPC_F32)
        return fail(LDPC_ERR_UNSUPPORTED, "the layered joint loss exists for fp32 decoders only (a float64 decoder has no layered schedule)");
    if (d->schedule == LDPC_SCHED_FLOODING && d->form == LDPC_C2V_RCQ)
        return fail(LDPC_ERR_UNSUPPORTED, "a flooding RCQ decoder takes ldpc_train_joint_ste, not ldpc_train_joint_layered");
    if (d->schedule == LDPC_SCHED_FLOODING)
        return fail(LDPC_ERR_UNSUPPORTED, "a flooding min-sum decoder takes ldpc_train_joint, not ldpc_train_joint_layered");
    if (d->form == LDPC_C2V_RCQ || d->schedule != LDPC_SCHED_LAYERED)
        return fail(LDPC_ERR_UNSUPPORTED, "the layered joint loss exists for the min-sum forms (LDPC_C2V_NMS / LDPC_C2V_OMS) under "
                                          "LDPC_SCHED_LAYERED; the RCQ decoder takes ldpc_train_joint_layered_ste under "
                                          "LDPC_SCHED_LAYERED and ldpc_train_joint_ste under flooding, the reference's layered "
                                          "schedule (LDPC_SCHED_LAYERED_REF) has no gradient path");
    return LDPC_OK;
}

struct JointWs {
    int vec = 0, tiles = 0;
    // every kind.  gedge: d J/d v2c_t (flooding) / d J/d u (layered)
    float *postT = nullptr, *yT = nullptr, *gllrT = nullptr, *gedge = nullptr, *gbeta = nullptr, *goa = nullptr;
    uint64_t *bitsT = nullptr;
    double *loss_part = nullptr, *item_sum = nullptr;
    // flooding: v2c / c2v are chosen per iteration (1-byte c2v rows for kJointSte)
    float *llrT = nullptr, *galpha = nullptr;
    char *v2c[2] = {nullptr, nullptr}, *c2v[2] = {nullptr, nullptr};
    // layered: the posterior copy g_l is formed on, R (kJointLayeredSte: 1-byte codes in its place), U
    float *glT = nullptr, *msgs = nullptr, *urows = nullptr;
    uint8_t *codes = nullptr;
    // the level-gradient entry points: level_grad's partials [tile][chunk][L] and their per-tile sums [tile][L]
    int lvl_chunks = 0;
    double *lvl_part = nullptr, *lvl_tile = nullptr;
    size_t total = 0;
};
JointWs carve_joint(const ldpc_decoder *d, int64_t batch, void *base, int kind, bool levels = false)
{
    JointWs w;
    const bool layered = kind == kJointLayered || kind == kJointLayeredSte;
    w.vec = layered ? 1 : pick_vec(d, batch);             // the layered walk is one wave per 64-codeword tile
    const int W = 64 * w.vec;
    w.tiles = (int)std::max<int64_t>((batch + W - 1) / W, 1);
    const size_t n = d->g->n, E = std::max(d->g->E, 1), tw = (size_t)w.tiles * W, tiles = w.tiles;
    const size_t vb = (n + kWavesPerBlock - 1) / kWavesPerBlock;
    const size_t nrow = tw * n * 4, erow = tw * E * 4, crow = tw * E * (kind == kJointSte ? 1 : 4);
    size_t off = 0;
    auto take = [&](auto *&p, size_t bytes) {
        if (base) p = reinterpret_cast<std::remove_reference_t<decltype(p)>>((char *)base + off);
        off += align_up(bytes);
    };
    // the rows in the order of the layouts the step times were measured with (the walk's P, R and U rows side by side)
    if (!layered) take(w.llrT, nrow);
    take(w.postT, nrow);
    if (layered) take(w.glT, nrow);
    take(w.yT, nrow); take(w.gllrT, nrow);
    if (kind == kJointLayeredSte) {
        take(w.codes, tw * E); take(w.urows, erow);
    } else if (layered) {
        take(w.msgs, erow); take(w.urows, erow);
    } else {
        take(w.v2c[0], erow); take(w.v2c[1], erow); take(w.c2v[0], crow); take(w.c2v[1], crow);
    }
    take(w.gedge, erow);
    take(w.bitsT, tiles * n * w.vec * sizeof(uint64_t));
    take(w.gbeta, tiles * E * 4); take(w.goa, d->form == LDPC_C2V_OMS ? tiles * E * 4 : 0);
    if (!layered) take(w.galpha, tiles * n * 4);
    take(w.loss_part, tiles * vb * sizeof(double));
    // item_sum: the longest row of partials reduced -- per edge, and per variable where the variable-side alpha has a gradient
    take(w.item_sum, (layered ? E : std::max(n, E)) * sizeof(double));
    if (levels) {                                     // after everything else: the other rows lie where they lie without it
        const size_t L = (size_t)std::max(d->n_levels, 1);
        w.lvl_chunks = (int)((E + kLgChunk - 1) / kLgChunk);
        take(w.lvl_part, tiles * w.lvl_chunks * L * sizeof(double));
        take(w.lvl_tile, tiles * L * sizeof(double));
    }
    w.total = off;
    return w;
}

// forward iteration t, flooding: the decode's own sweeps (fixed T, no stop latch); the variable sweep keeps l_t in postT
template <int VEC>
int joint_forward_flooding(const ldpc_decoder *d, const JointWs &w, int t, bool last, hipStream_t s)
{
    Workspace wc;
    wc.vec = w.vec; wc.tiles = w.tiles;
    wc.llrT = (char *)w.llrT; wc.postT = (char *)w.postT; wc.bitsT = w.bitsT;
    Workspace wv = wc;
    wc.v2c = w.v2c[t & 1]; wc.c2v = w.c2v[t & 1];
    wv.c2v = w.c2v[t & 1]; wv.v2c = w.v2c[(t + 1) & 1];
    if (int rc = launch_cn<float, VEC>(d, wc, t, /*use_done=*/false, s)) return rc;
    return launch_vn<float, VEC>(d, wv, t, last, /*use_done=*/false, s, /*store_posterior=*/true, nullptr, /*keep_posterior=*/true);
}

// forward iteration t, layered (VEC = 1): one walk over the checks, a wave per tile; P_t in postT, u of every edge in urows
void joint_forward_layered(const ldpc_decoder *d, const JointWs &w, int t, uint64_t *bitsT, hipStream_t s)
{
    const GraphDev g = d->g->dev();
    const float *beta_row = (const float *)d->beta + (size_t)t * d->n_beta;
    if (d->form == LDPC_C2V_RCQ) {      // the quantiser of this iteration, and the one that wrote the codes it subtracts
        const float *thr = d->thresholds + (size_t)d->q_of_iter[t] * d->n_levels;
        const float *thr_prev = d->thresholds + (size_t)d->q_of_iter[t > 0 ? t - 1 : 0] * d->n_levels;
        hipLaunchKernelGGL((layered_rcq_iter<1>), dim3(w.tiles), dim3(kWave), 0, s, g, w.postT, w.codes, w.urows, beta_row,
                           (const int *)d->beta_slot, thr, thr_prev, d->n_levels, t == 0 ? 1 : 0, d->g->max_dc, bitsT);
    } else if (d->form == LDPC_C2V_OMS) {
        const float *oa_row = d->oms_alpha ? (const float *)d->oms_alpha + (size_t)t * d->n_oms_alpha : nullptr;
        hipLaunchKernelGGL((layered_minsum_iter<1, FORM_OMS>), dim3(w.tiles), dim3(kWave), 0, s, g, w.postT, w.msgs, w.urows,
                           beta_row, (const int *)d->beta_slot, oa_row, (const int *)d->oms_alpha_slot, bitsT);
    } else {
        hipLaunchKernelGGL((layered_minsum_iter<1, FORM_NMS>), dim3(w.tiles), dim3(kWave), 0, s, g, w.postT, w.msgs, w.urows,
                           beta_row, (const int *)d->beta_slot, (const float *)nullptr, (const int *)nullptr, bitsT);
    }
}

template <int VEC>
int joint_impl(const ldpc_decoder *d, const float *llr, const float *targets, int64_t batch, const float *weights,
               float *loss_per_iter, int32_t *bits, float *posterior, float *grad_beta, float *grad_alpha,
               float *grad_oms_alpha, float *grad_llr, float *grad_levels, const JointWs &w, int kind, hipStream_t s)
{
    constexpr int W = 64 * VEC;
    constexpr int JT = transpose_vars<float>();
    const GraphDev g = d->g->dev();
    const int T = d->T, tiles = w.tiles, vc = (g.n + JT - 1) / JT;
    const dim3 tgrid((unsigned)((size_t)tiles * VEC * vc)), blk(kBlock);
    const bool layered = kind == kJointLayered || kind == kJointLayeredSte, oms = d->form == LDPC_C2V_OMS, rcq = d->form == LDPC_C2V_RCQ;
    const bool want_tables = grad_beta || grad_alpha || grad_oms_alpha || grad_llr;
    const bool want = want_tables || grad_levels;     // the seed g_t is formed for either
    const bool oa_grad = grad_oms_alpha && oms && d->oms_alpha;
    const size_t nrow_bytes = (size_t)tiles * W * g.n * sizeof(float);
    // flooding: the LLR rows stay; layered: P = llr, R = +0 ("no message yet"; the RCQ walk reads no code in iteration 0),
    // as the decode starts
    hipLaunchKernelGGL((transpose_in<float, VEC>), tgrid, blk, 0, s, llr, layered ? w.postT : w.llrT, (long long)batch, g.n, vc);
    if (targets)
        hipLaunchKernelGGL((transpose_in<float, VEC>), tgrid, blk, 0, s, targets, w.yT, (long long)batch, g.n, vc);
    if (kind == kJointLayered) HIP_TRY(hipMemsetAsync(w.msgs, 0, (size_t)tiles * W * g.E * sizeof(float), s));
    // rows no step writes: alpha_T-1, and every alpha row where the variable update has no parameter (the offset forms,
    // the layered schedule)
    if (grad_alpha) {
        const size_t row = (size_t)d->n_alpha * 4;
        if (oms || layered) HIP_TRY(hipMemsetAsync(grad_alpha, 0, (size_t)T * row, s));
        else HIP_TRY(hipMemsetAsync((char *)grad_alpha + (size_t)(T - 1) * row, 0, row, s));
    }
    if (grad_oms_alpha && !oa_grad && d->n_oms_alpha > 0)
        HIP_TRY(hipMemsetAsync(grad_oms_alpha, 0, (size_t)T * d->n_oms_alpha * 4, s));
    if (grad_llr) HIP_TRY(hipMemsetAsync(w.gllrT, 0, nrow_bytes, s));
    const int cb = (g.m + kWavesPerBlock - 1) / kWavesPerBlock, vb = (g.n + kWavesPerBlock - 1) / kWavesPerBlock;
    const int vbb = (g.n + kWavesPerBlock * kVnbVarsPerWave - 1) / (kWavesPerBlock * kVnbVarsPerWave);
    const dim3 cgrid((unsigned)((size_t)tiles * cb)), vgrid((unsigned)((size_t)tiles * vb)), vbgrid((unsigned)((size_t)tiles * vbb));
    const double inv_bn = 1.0 / ((double)batch * (double)g.n);
    const float *yT = targets ? w.yT : nullptr;
    // one iteration's partials [tile][item] -> its row of a gradient table: per-item sums over the tiles, then per slot
    auto reduce_step = [&](const float *part, int count, const int *slot_ptr, const int *slot_items, int n_slots, float *row) {
        hipLaunchKernelGGL(reduce_tiles, dim3((unsigned)((count + kBlock - 1) / kBlock)), blk, 0, s, part, tiles, count, w.item_sum);
        hipLaunchKernelGGL(reduce_table_grads<double>, dim3((unsigned)n_slots), dim3(kWave), 0, s, (const double *)w.item_sum, 1,
                           count, slot_ptr, slot_items, n_slots, row);
    };
    for (int t = 0; t < T; ++t) {
        const bool last = t == T - 1;
        if (!layered) {
            if (int rc = joint_forward_flooding<VEC>(d, w, t, last, s)) return rc;
        } else if constexpr (VEC == 1) {
            joint_forward_layered(d, w, t, (last && bits) ? w.bitsT : nullptr, s);
        }   // no layered step in joint_impl<4>: carve_joint gives the layered kind vec = 1, so train_joint_entry never asks for it
        if (last && (bits || posterior))
            hipLaunchKernelGGL((transpose_out<float, VEC>), tgrid, blk, 0, s, (const float *)w.postT, (const uint64_t *)w.bitsT,
                               posterior, bits, (long long)batch, g.n, vc);
        // J_t, and with a gradient its seed g_l, written in place: over postT (flooding: the next sweeps do not read it), over a
        // copy of the posterior rows (layered: the walk goes on with P)
        float *seed = w.postT;
        if (layered && want) {
            seed = w.glT;
            HIP_TRY(hipMemcpyAsync(w.glT, w.postT, nrow_bytes, hipMemcpyDeviceToDevice, s));
        }
        if (want)
            hipLaunchKernelGGL((joint_loss_grad<VEC, true>), vgrid, blk, 0, s, g.n, seed, yT, weights, t, (long long)batch,
                               (float)inv_bn, grad_llr ? w.gllrT : nullptr, w.loss_part, vb);
        else
            hipLaunchKernelGGL((joint_loss_grad<VEC, false>), vgrid, blk, 0, s, g.n, seed, yT, weights, t, (long long)batch,
                               (float)inv_bn, (float *)nullptr, w.loss_part, vb);
        hipLaunchKernelGGL(joint_loss_reduce, dim3(1), blk, 0, s, (const double *)w.loss_part, (long long)tiles * vb, inv_bn,
                           loss_per_iter + t);
        HIP_TRY(hipGetLastError());
        if (!want) continue;
        if (grad_levels) {
            // d J_t/d tau: the seed against the codes of iteration t (flooding: this iteration's check sweep; layered: after
            // the walk every code in the rows is this iteration's), into row t
            const uint8_t *lcodes = layered ? (const uint8_t *)w.codes : (const uint8_t *)w.c2v[t & 1];
            const int L = d->n_levels, waves = tiles * w.lvl_chunks;
#define LDPC_LVG(NREG_, BLOCK_, LDS_)                                                                                  \
    hipLaunchKernelGGL((level_grad<VEC, NREG_>), dim3((unsigned)((waves + (BLOCK_) / kWave - 1) / ((BLOCK_) / kWave))),    \
                       dim3(BLOCK_), (size_t)(LDS_), s, g, lcodes, (const float *)seed, (long long)batch, L, w.lvl_chunks, \
                       waves, w.lvl_part)
            if (L <= 4) LDPC_LVG(4, kBlock, 0);
            else if (L <= 8) LDPC_LVG(8, kBlock, 0);
            else LDPC_LVG(0, kWave, (size_t)L * kWave * sizeof(float));
#undef LDPC_LVG
            hipLaunchKernelGGL(level_grad_waves, dim3((unsigned)((tiles * L + kBlock - 1) / kBlock)), blk, 0, s,
                               (const double *)w.lvl_part, tiles, w.lvl_chunks, L, w.lvl_tile);
            hipLaunchKernelGGL(reduce_table_grads<double>, dim3((unsigned)L), dim3(kWave), 0, s, (const double *)w.lvl_tile,
                               tiles, L, (const int *)d->level_iota, (const int *)d->level_iota, L,
                               grad_levels + (size_t)t * L);
            HIP_TRY(hipGetLastError());
        }
        if (!want_tables) continue;
        // posterior-local backward of iteration t: check side (beta_t, offset alpha_t, d J/d v2c_t or d J/d u), then the
        // alpha_t-1 partial of the flooding normalised / RCQ forms and the LLR gradient
        const bool alpha_step = !layered && !oms && t >= 1 && grad_alpha;
        const bool first = !layered && t == 0;            // v2c_0 = llr; the layered u rows are messages in every iteration
        const float *src = layered ? w.urows : first ? w.llrT : (const float *)w.v2c[t & 1];
        const uint8_t *codes = !rcq ? nullptr : layered ? (const uint8_t *)w.codes : (const uint8_t *)w.c2v[t & 1];
        const float *beta_row = (const float *)d->beta + (size_t)t * d->n_beta;
        float *gedge_out = (grad_llr || alpha_step) ? w.gedge : nullptr;
        float *goa = oa_grad ? w.goa : nullptr;
        // codes / n_levels: read by FORM_RCQ alone; nullptr / 0 for the min-sum forms (n_levels is set for RCQ decoders only)
#define LDPC_CNJ(FIRST_, FORM_, SRC_, SEED_, CODES_)                                                                   \
    hipLaunchKernelGGL((cn_backward<VEC, FIRST_, FORM_, true>), cgrid, blk, 0, s, g, (const float *)(SRC_),            \
                       (const float *)nullptr, (const float *)(SEED_), (const int *)nullptr, (long long)batch, t,     \
                       beta_row, (const int *)d->beta_slot, gedge_out, w.gbeta, goa, cb, (const uint8_t *)(CODES_),    \
                       d->n_levels)
        if (first) {
            if (oms) LDPC_CNJ(true, FORM_OMS, src, seed, codes); else if (rcq) LDPC_CNJ(true, FORM_RCQ, src, seed, codes);
            else LDPC_CNJ(true, FORM_NMS, src, seed, codes);
        } else {
            if (oms) LDPC_CNJ(false, FORM_OMS, src, seed, codes); else if (rcq) LDPC_CNJ(false, FORM_RCQ, src, seed, codes);
            else LDPC_CNJ(false, FORM_NMS, src, seed, codes);
        }
#undef LDPC_CNJ
        if (grad_beta) reduce_step(w.gbeta, g.E, d->beta_inv_ptr, d->beta_inv_items, d->n_beta, grad_beta + (size_t)t * d->n_beta);
        if (oa_grad)
            reduce_step(w.goa, g.E, d->oms_inv_ptr, d->oms_inv_items, d->n_oms_alpha, grad_oms_alpha + (size_t)t * d->n_oms_alpha);
        if (alpha_step) {
            const float *alpha_row = (const float *)d->alpha + (size_t)(t - 1) * d->n_alpha;
            if (rcq) {                                    // code rows of iteration t-1, reconstructed with ITS quantiser
                const int lut_entries = 2 * d->n_levels;
                hipLaunchKernelGGL((vn_backward<VEC, true, true>), vbgrid, blk, 0, s, g, (const void *)w.c2v[(t - 1) & 1],
                                   (const float *)w.gedge, (const int *)nullptr, (long long)batch, t, alpha_row,
                                   (const int *)d->alpha_slot, (float *)nullptr, w.galpha, vbb,
                                   (const float *)d->lut + (size_t)d->q_of_iter[t - 1] * lut_entries, lut_entries);
            } else {
                hipLaunchKernelGGL((vn_backward<VEC, true>), vbgrid, blk, 0, s, g, (const void *)w.c2v[(t - 1) & 1],
                                   (const float *)w.gedge, (const int *)nullptr, (long long)batch, t, alpha_row,
                                   (const int *)d->alpha_slot, (float *)nullptr, w.galpha, vbb);
            }
            reduce_step(w.galpha, g.n, d->alpha_inv_ptr, d->alpha_inv_items, d->n_alpha, grad_alpha + (size_t)(t - 1) * d->n_alpha);
        }
        if (grad_llr)         // d J_t/d llr_v = g_t[v] + the sum over the edges of v of d J_t/d v2c_t (layered: u_e = llr_v + const)
            hipLaunchKernelGGL((llr_backward_accumulate<VEC>), vgrid, blk, 0, s, g, (const float *)w.gedge, w.gllrT, vb);
        HIP_TRY(hipGetLastError());
    }
    if (grad_llr)
        hipLaunchKernelGGL((transpose_out<float, VEC>), tgrid, blk, 0, s, (const float *)w.gllrT, (const uint64_t *)nullptr, grad_llr,
                           (int *)nullptr, (long long)batch, g.n, vc);
    HIP_TRY(hipGetLastError());
    return LDPC_OK;
}

size_t joint_workspace_bytes(const ldpc_decoder *d, int64_t batch, int kind, bool levels = false)
{
    if (!d || batch < 0) return 0;
    if (levels && d->form != LDPC_C2V_RCQ) return 0;      // no levels: the entry point refuses such a decoder
    return carve_joint(d, batch, nullptr, kind, levels).total;
}

// ldpc_train_joint, ldpc_train_joint_ste, ldpc_train_joint_layered and ldpc_train_joint_layered_ste: the same argument rules
int train_joint_entry(const ldpc_decoder *d, int kind, const void *llr, const void *targets, int64_t batch,
                      const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                      void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr, void *workspace,
                      size_t workspace_bytes, void *stream, bool levels = false, void *grad_levels = nullptr)
{
    const bool ste = kind == kJointSte, layered = kind == kJointLayered || kind == kJointLayeredSte;
    if (int rc = joint_supported(d, kind)) return rc;
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (d->T < 1) return fail(LDPC_ERR_UNSUPPORTED, "the joint loss needs at least one iteration");
    if (!d->beta_inv_ptr || (!layered && !d->alpha_inv_ptr)) return fail(LDPC_ERR_UNSUPPORTED, "internal: the decoder has no inverse slot maps");
    if (ste && d->n_levels > kVnbLutMax / 2) return fail(LDPC_ERR_UNSUPPORTED, "more than %d quantiser levels", kVnbLutMax / 2);
    if (!loss_per_iter) return fail(LDPC_ERR_ARG, "NULL loss_per_iter");
    const bool want = grad_beta || grad_alpha || grad_oms_alpha || grad_llr || grad_levels;
    if (want && !iteration_weights) return fail(LDPC_ERR_ARG, "NULL iteration_weights");
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    if (batch == 0) {                                 // an empty batch: every loss term and every gradient is 0
        HIP_TRY(hipMemsetAsync(loss_per_iter, 0, (size_t)d->T * 4, s));
        if (grad_beta) HIP_TRY(hipMemsetAsync(grad_beta, 0, (size_t)d->T * d->n_beta * 4, s));
        if (grad_alpha) HIP_TRY(hipMemsetAsync(grad_alpha, 0, (size_t)d->T * d->n_alpha * 4, s));
        if (grad_oms_alpha && d->n_oms_alpha > 0) HIP_TRY(hipMemsetAsync(grad_oms_alpha, 0, (size_t)d->T * d->n_oms_alpha * 4, s));
        if (grad_levels) HIP_TRY(hipMemsetAsync(grad_levels, 0, (size_t)d->T * d->n_levels * 4, s));
        return LDPC_OK;
    }
    if (d->g->n == 0 || d->g->E == 0) return fail(LDPC_ERR_UNSUPPORTED, "the joint loss needs a graph with edges");
    if (!llr || !workspace) return fail(LDPC_ERR_ARG, "NULL llr/workspace");
    if (((uintptr_t)workspace % kAlign) != 0) return fail(LDPC_ERR_ARG, "workspace must be %zu-byte aligned", kAlign);
    const JointWs w = carve_joint(d, batch, workspace, kind, levels);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    if ((size_t)w.tiles * ((d->g->n + 3) / 4) > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
#define LDPC_JOINT(V_)                                                                                                 \
    joint_impl<V_>(d, (const float *)llr, (const float *)targets, batch, (const float *)iteration_weights,             \
                   (float *)loss_per_iter, bits, (float *)posterior, (float *)grad_beta, (float *)grad_alpha,          \
                   (float *)grad_oms_alpha, (float *)grad_llr, (float *)grad_levels, w, kind, s)
    if (w.vec == 1) return LDPC_JOINT(1);
    return LDPC_JOINT(4);
#undef LDPC_JOINT
}
}  // namespace

extern "C" {

size_t ldpc_train_saved_bytes(const ldpc_decoder *d, int64_t batch)
{
    if (!d || batch <= 0) return 0;
    const int vec = pick_vec(d, batch), W = 64 * vec;
    const size_t total = saved_layout(d, (int)((batch + W - 1) / W), W).total();
    return total ? total : kAlign;
}

size_t ldpc_train_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    if (!d || batch < 0) return 0;
    return std::max(carve(d, batch, nullptr).total, carve_backward(d, batch, nullptr).total);
}

int ldpc_decode_saving(const ldpc_decoder *d, const void *llr, int64_t batch, int32_t early_stop, int32_t *bits,
                       void *posterior, int32_t *iterations, uint8_t *success, void *saved, size_t saved_bytes,
                       void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = train_supported(d)) return rc;
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (batch == 0 || d->g->n == 0) return LDPC_OK;
    if (!llr || !workspace || !saved) return fail(LDPC_ERR_ARG, "NULL llr/workspace/saved");
    if (((uintptr_t)workspace % kAlign) != 0 || ((uintptr_t)saved % kAlign) != 0)
        return fail(LDPC_ERR_ARG, "workspace and saved state must be %zu-byte aligned", kAlign);
    const Workspace w = carve(d, batch, workspace);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    if (ldpc_train_saved_bytes(d, batch) > saved_bytes) return fail(LDPC_ERR_WORKSPACE, "saved-state buffer too small");
    if ((size_t)w.tiles * ((d->g->n + 3) / 4) > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    DeviceGuard guard(d->g->device);
    return decode_dispatch<float>(d, llr, batch, early_stop != 0, bits, posterior, iterations, success, nullptr, w,
                                  (hipStream_t)stream, (char *)saved);
}

int ldpc_backward(const ldpc_decoder *d, const void *saved, size_t saved_bytes, const void *llr, int64_t batch,
                  const int32_t *iterations, const void *grad_posterior, void *grad_beta, void *grad_alpha,
                  void *grad_oms_alpha, void *grad_llr, void *workspace, size_t workspace_bytes, void *stream)
{
    if (int rc = train_supported(d)) return rc;
    if (batch < 0) return fail(LDPC_ERR_ARG, "batch < 0");
    if (!grad_beta && !grad_alpha && !grad_oms_alpha && !grad_llr) return LDPC_OK;
    DeviceGuard guard(d->g->device);
    hipStream_t s = (hipStream_t)stream;
    if (batch == 0 || d->g->n == 0 || d->T == 0 || d->g->E == 0) {       // no iteration ran: the posterior is the LLR
        if (grad_beta) HIP_TRY(hipMemsetAsync(grad_beta, 0, (size_t)std::max(d->T, 1) * d->n_beta * 4, s));
        if (grad_alpha) HIP_TRY(hipMemsetAsync(grad_alpha, 0, (size_t)std::max(d->T, 1) * d->n_alpha * 4, s));
        if (grad_oms_alpha && d->n_oms_alpha > 0)
            HIP_TRY(hipMemsetAsync(grad_oms_alpha, 0, (size_t)std::max(d->T, 1) * d->n_oms_alpha * 4, s));
        if (grad_llr && batch > 0 && d->g->n > 0) {              // no iteration ran: posterior == llr
            if (!grad_posterior) return fail(LDPC_ERR_ARG, "NULL grad_posterior");
            HIP_TRY(hipMemcpyAsync(grad_llr, grad_posterior, (size_t)batch * d->g->n * 4, hipMemcpyDeviceToDevice, s));
        }
        return LDPC_OK;
    }
    if (!saved || !llr || !iterations || !grad_posterior || !workspace) return fail(LDPC_ERR_ARG, "NULL argument");
    if (((uintptr_t)workspace % kAlign) != 0 || ((uintptr_t)saved % kAlign) != 0)
        return fail(LDPC_ERR_ARG, "workspace and saved state must be %zu-byte aligned", kAlign);
    if (ldpc_train_saved_bytes(d, batch) > saved_bytes) return fail(LDPC_ERR_WORKSPACE, "saved-state buffer too small");
    const BackwardWs w = carve_backward(d, batch, workspace);
    if (w.total > workspace_bytes) return fail(LDPC_ERR_WORKSPACE, "workspace %zu < required %zu", workspace_bytes, w.total);
    if ((size_t)w.tiles * ((d->g->n + 3) / 4) > 0x7fffffffull) return fail(LDPC_ERR_UNSUPPORTED, "batch too large for one launch");
    if (w.vec == 1)
        return backward_impl<1>(d, (const char *)saved, (const float *)llr, batch, iterations, (const float *)grad_posterior,
                                (float *)grad_beta, (float *)grad_alpha, (float *)grad_oms_alpha, (float *)grad_llr, w, s);
    return backward_impl<4>(d, (const char *)saved, (const float *)llr, batch, iterations, (const float *)grad_posterior,
                            (float *)grad_beta, (float *)grad_alpha, (float *)grad_oms_alpha, (float *)grad_llr, w, s);
}


size_t ldpc_train_joint_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointMinsum);
}

int ldpc_train_joint(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                     const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                     void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr, void *workspace,
                     size_t workspace_bytes, void *stream)
{
    return train_joint_entry(d, kJointMinsum, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior, grad_beta,
                             grad_alpha, grad_oms_alpha, grad_llr, workspace, workspace_bytes, stream);
}

size_t ldpc_train_joint_ste_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointSte);
}

int ldpc_train_joint_ste(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                         const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                         void *grad_beta, void *grad_alpha, void *grad_llr, void *workspace, size_t workspace_bytes,
                         void *stream)
{
    return train_joint_entry(d, kJointSte, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior, grad_beta,
                             grad_alpha, nullptr, grad_llr, workspace, workspace_bytes, stream);
}

size_t ldpc_train_joint_layered_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointLayered);
}

int ldpc_train_joint_layered(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                             const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                             void *grad_beta, void *grad_alpha, void *grad_oms_alpha, void *grad_llr, void *workspace,
                             size_t workspace_bytes, void *stream)
{
    return train_joint_entry(d, kJointLayered, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior,
                             grad_beta, grad_alpha, grad_oms_alpha, grad_llr, workspace, workspace_bytes, stream);
}

size_t ldpc_train_joint_layered_ste_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointLayeredSte);
}

int ldpc_train_joint_layered_ste(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                 const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                 void *grad_beta, void *grad_alpha, void *grad_llr, void *workspace,
                                 size_t workspace_bytes, void *stream)
{
    return train_joint_entry(d, kJointLayeredSte, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior,
                             grad_beta, grad_alpha, nullptr, grad_llr, workspace, workspace_bytes, stream);
}

size_t ldpc_train_joint_ste_levels_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointSte, true);
}

int ldpc_train_joint_ste_levels(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                void *grad_beta, void *grad_alpha, void *grad_llr, void *grad_levels, void *workspace,
                                size_t workspace_bytes, void *stream)
{
    return train_joint_entry(d, kJointSte, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior, grad_beta,
                             grad_alpha, nullptr, grad_llr, workspace, workspace_bytes, stream, true, grad_levels);
}

size_t ldpc_train_joint_layered_ste_levels_workspace_bytes(const ldpc_decoder *d, int64_t batch)
{
    return joint_workspace_bytes(d, batch, kJointLayeredSte, true);
}

int ldpc_train_joint_layered_ste_levels(const ldpc_decoder *d, const void *llr, const void *targets, int64_t batch,
                                        const void *iteration_weights, void *loss_per_iter, int32_t *bits, void *posterior,
                                        void *grad_beta, void *grad_alpha, void *grad_llr, void *grad_levels,
                                        void *workspace, size_t workspace_bytes, void *stream)
{
    return train_joint_entry(d, kJointLayeredSte, llr, targets, batch, iteration_weights, loss_per_iter, bits, posterior,
                             grad_beta, grad_alpha, nullptr, grad_llr, workspace, workspace_bytes, stream, true, grad_levels);
}

}  // extern "C"
