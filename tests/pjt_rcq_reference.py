"""
CPU restatement of posterior joint training of the quantised decoder (W-RCQ, straight-through estimator), the semantics
``WeightedRCQDecoder.joint_posterior_loss(quantizer_gradient="straight_through")`` / ldpc_train_joint_ste pin.

The structure of tests/pjt_reference.py (same padded gathers, same tie rules for min / min2, same sign(0) and degree-1
handling, the same stop-gradient on the leave-one-out sum, the same loss), with the check output of iteration t formed as
        c2v_t = deq.detach() + mask * (m - m.detach()),     m = beta_t[slot(e)] * (minval * prod of the other signs)
where  deq  = Q_t^-1(code_t[e])  and  mask = (code_t[e] mod L) < L - 1  are taken from the codes a fixed-T decode wrote.

TEACHER-FORCED: the codes are those of ``oracle.decode(..., early_stop=False, trace_codes=True)`` (uint8 [B, T, E]), which
the parity tests pin bit for bit against the kernels.  A quantiser is discontinuous: a free-running fp32 restatement would
flip a code in a few batches and make a gradient comparison meaningless.  So that the forcing cannot hide a wrong
restatement, ``forward`` also quantises its own ``m`` in torch and returns the share of (b, t, e) triples on which that
disagrees with the traced code; the tests bound it.
Torch autograd on this graph is the reference gradient of the tests.  Test infrastructure, not product code.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from grad_oracle import _padded_neighbourhoods


def trace(g, llr, beta_table, beta_slot, alpha_table, alpha_slot, thresholds, q_of_iter, T):
    """the fixed-T decode of the CPU oracle -> (bits [B, n], posterior [B, n], codes uint8 [B, T, E])"""
    import oracle
    bits, post, _, _, codes = oracle.decode(
        g, np.ascontiguousarray(llr, dtype=np.float32), T=T, early_stop=False, c2v_form=oracle.C2V_RCQ,
        sum_order=oracle.SUM_TORCH, beta=np.asarray(beta_table, np.float32), beta_slot=beta_slot,
        alpha=np.asarray(alpha_table, np.float32), alpha_slot=alpha_slot, thresholds=thresholds, q_of_iter=q_of_iter,
        trace_codes=True)
    return bits, post, codes


def forward(g, llr, codes, beta_table, beta_slot, alpha_table, alpha_slot, thresholds, q_of_iter, T, targets=None,
            weights=None, dtype=torch.float32):
    """llr [B, n], beta_table [T, Sb], alpha_table [T, Sa] torch tensors (may require grad); codes uint8 [B, T, E] of the
    fixed-T decode; thresholds float32 [Q, L], q_of_iter [T].  -> (J, [J_t], final posterior [B, n], disagreement share)"""
    B, n = llr.shape
    E = g.E
    thr = torch.from_numpy(np.asarray(thresholds, dtype=np.float32))
    L = thr.shape[1]
    codes = torch.from_numpy(np.asarray(codes)).to(torch.long)
    y = torch.zeros(B, n, dtype=dtype) if targets is None else torch.as_tensor(targets, dtype=dtype)
    w = torch.full((T,), 1.0 / T, dtype=dtype) if weights is None else torch.as_tensor(weights, dtype=dtype)
    ce, ve = _padded_neighbourhoods(g)
    cmask = ce < E
    var_of_edge = torch.from_numpy(g.var_idx.astype(np.int64))
    bslot = torch.from_numpy(np.asarray(beta_slot, dtype=np.int64))
    aslot_e = torch.from_numpy(np.asarray(alpha_slot, dtype=np.int64))[var_of_edge]
    dc = torch.from_numpy(g.dc.astype(np.int64))
    chk_of_edge = torch.from_numpy(g.rows.astype(np.int64))
    pos_of_edge = torch.arange(E) - torch.from_numpy(g.check_ptr.astype(np.int64))[chk_of_edge]
    kpos = np.empty(E, dtype=np.int64)
    kpos[g.csc_edge] = np.arange(E) - np.repeat(g.var_ptr[:-1].astype(np.int64), g.dv)
    kpos_of_edge = torch.from_numpy(kpos)
    max_dc, max_dv = ce.shape[1], ve.shape[1]
    eye_c = torch.eye(max_dc, dtype=torch.bool)
    eye_v = torch.eye(max_dv, dtype=torch.bool)
    inf = torch.tensor(float("inf"), dtype=dtype)

    v2c = llr[:, var_of_edge]
    J = torch.zeros((), dtype=dtype)
    per_iter = []
    post = llr
    differ = 0
    for t in range(T):
        tau = thr[int(q_of_iter[t])]                          # float32 [L]: the quantiser of THIS iteration
        pad = torch.cat([v2c, torch.zeros(B, 1, dtype=dtype)], dim=1)
        inc = pad[:, ce]
        mags = torch.where(cmask, inc.abs(), inf)
        signs = torch.where(cmask, torch.sign(inc), torch.ones((), dtype=dtype))
        m1, i1 = mags.min(dim=-1, keepdim=True)
        m2 = mags.scatter(-1, i1, float("inf")).amin(dim=-1, keepdim=True)
        m2 = torch.where((dc == 1).view(1, -1, 1), m1, m2)
        pos = torch.arange(max_dc).view(1, 1, -1)
        minval = torch.where(pos == i1, m2, m1)
        s_others = torch.where(eye_c.view(1, 1, max_dc, max_dc), torch.ones((), dtype=dtype), signs.unsqueeze(-2))
        prod_others = s_others.prod(dim=-1)
        beta_e = beta_table[t][bslot]
        alpha_e = alpha_table[t][aslot_e]
        m = beta_e.view(1, -1) * (minval * prod_others)[:, chk_of_edge, pos_of_edge]
        # the forward's value and the straight-through mask, both from the code the decode wrote
        code = codes[:, t, :]
        level = code % L
        deq = ((1.0 - 2.0 * (code >= L).to(torch.float32)) * tau[level]).to(dtype)
        mask = (level < L - 1).to(dtype)
        c2v = deq.detach() + mask * (m - m.detach())
        # this restatement's own quantiser on its own m (rcq_decoder.py:79-89): level = last q with |m| >= tau_q
        md = m.detach()
        own = torch.zeros_like(code)
        for q in range(L):
            own = torch.where(md.abs() >= tau[q].to(dtype), torch.full_like(own, q), own)
        own = own + (md < 0).to(torch.long) * L
        differ += int((own != code).sum())
        at_var = torch.cat([c2v, torch.zeros(B, 1, dtype=dtype)], dim=1)[:, ve]
        post = llr + at_var.sum(dim=-1)
        Jt = F.binary_cross_entropy_with_logits(-post, y)
        per_iter.append(Jt)
        J = J + w[t] * Jt
        others = torch.where(eye_v.view(1, 1, max_dv, max_dv), torch.zeros((), dtype=dtype),
                             at_var.unsqueeze(-2)).sum(dim=-1)
        loo = others[:, var_of_edge, kpos_of_edge].detach()                  # the stop-gradient of PJT
        v2c = llr[:, var_of_edge] + alpha_e.view(1, -1) * loo
    return J, per_iter, post, differ / max(B * T * E, 1)


def joint_grads(g, llr, codes, beta_table, beta_slot, alpha_table, alpha_slot, thresholds, q_of_iter, T, targets=None,
                weights=None, want_llr=False, dtype=torch.float32):
    """-> dict(loss, loss_per_iter [T], grad_beta [T, Sb], grad_alpha [T, Sa], posterior, disagree[, grad_llr]) as numpy"""
    bt = torch.tensor(np.asarray(beta_table), dtype=dtype, requires_grad=True)
    at = torch.tensor(np.asarray(alpha_table), dtype=dtype, requires_grad=True)
    x = torch.tensor(np.asarray(llr), dtype=dtype, requires_grad=want_llr)
    J, per_iter, post, disagree = forward(g, x, codes, bt, beta_slot, at, alpha_slot, thresholds, q_of_iter, T, targets,
                                          weights, dtype)
    wrt = (bt, at, x) if want_llr else (bt, at)
    grads = torch.autograd.grad(J, wrt, allow_unused=True)
    grads = [torch.zeros_like(v) if gr is None else gr for gr, v in zip(grads, wrt)]
    out = {"loss": float(J.detach()), "loss_per_iter": np.array([float(v.detach()) for v in per_iter]),
           "grad_beta": grads[0].numpy(), "grad_alpha": grads[1].numpy(), "posterior": post.detach().numpy(),
           "disagree": disagree}
    if want_llr:
        out["grad_llr"] = grads[2].numpy()
    return out
