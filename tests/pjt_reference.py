"""
CPU restatement of posterior joint training (PJT), the semantics ``joint_posterior_loss`` / ldpc_train_joint pin.

Built on the structure of oracle/grad_oracle.forward (same padded gathers, same tie rules for min / min2, same
sign(0) and degree-1 handling), with three changes:
  * fixed T = max_iterations, no early stop;
  * the leave-one-out C2V sum of the variable update is detached (the one stop-gradient of PJT):
        NMS:  v2c_{t+1}[e] = x_v + alpha_t[slot(v)] * sg(sum_{e' != e at v} c2v_t[e'])
        OMS:  v2c_{t+1}[e] = x_v + sg(sum_{e' != e at v} c2v_t[e'])
  * the loss is J = sum_t w_t * mean_{b, j} BCEWithLogits(-l_t[b, j], y[b, j]) over every iteration's posterior l_t.
Torch autograd on this graph is the reference gradient of the tests.  Test infrastructure, not product code.
"""

from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from grad_oracle import _padded_neighbourhoods


def forward(g, llr, beta_table, beta_slot, alpha_table, alpha_slot, T, targets=None, weights=None, offset=False,
            dtype=torch.float32):
    """llr [B, n], beta_table [T, Sb], alpha_table [T, Sa] torch tensors (may require grad); offset as in
    grad_oracle.forward (alpha per EDGE, check-side).  -> (J, [J_t], final posterior [B, n])"""
    B, n = llr.shape
    E = g.E
    y = torch.zeros(B, n, dtype=dtype) if targets is None else torch.as_tensor(targets, dtype=dtype)
    w = torch.full((T,), 1.0 / T, dtype=dtype) if weights is None else torch.as_tensor(weights, dtype=dtype)
    ce, ve = _padded_neighbourhoods(g)
    cmask = ce < E
    var_of_edge = torch.from_numpy(g.var_idx.astype(np.int64))
    bslot = torch.from_numpy(np.asarray(beta_slot, dtype=np.int64))
    aslot_e = torch.from_numpy(np.asarray(alpha_slot, dtype=np.int64))
    if not offset:
        aslot_e = aslot_e[var_of_edge]
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
    for t in range(T):
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
        if offset:
            raw = minval[:, chk_of_edge, pos_of_edge]
            c2v = prod_others[:, chk_of_edge, pos_of_edge] * (torch.relu(raw - beta_e.view(1, -1)) - alpha_e.view(1, -1))
        else:
            c2v = beta_e.view(1, -1) * (minval * prod_others)[:, chk_of_edge, pos_of_edge]
        at_var = torch.cat([c2v, torch.zeros(B, 1, dtype=dtype)], dim=1)[:, ve]
        post = llr + at_var.sum(dim=-1)
        Jt = F.binary_cross_entropy_with_logits(-post, y)
        per_iter.append(Jt)
        J = J + w[t] * Jt
        others = torch.where(eye_v.view(1, 1, max_dv, max_dv), torch.zeros((), dtype=dtype),
                             at_var.unsqueeze(-2)).sum(dim=-1)
        loo = others[:, var_of_edge, kpos_of_edge].detach()                  # the stop-gradient of PJT
        v2c = llr[:, var_of_edge] + (loo if offset else alpha_e.view(1, -1) * loo)
    return J, per_iter, post


def joint_grads(g, llr, beta_table, beta_slot, alpha_table, alpha_slot, T, targets=None, weights=None, offset=False,
                want_llr=False, dtype=torch.float32):
    """-> dict(loss, loss_per_iter [T], grad_beta [T, Sb], grad_alpha [T, Sa], posterior[, grad_llr]) as numpy"""
    bt = torch.tensor(np.asarray(beta_table), dtype=dtype, requires_grad=True)
    at = torch.tensor(np.asarray(alpha_table), dtype=dtype, requires_grad=True)
    x = torch.tensor(np.asarray(llr), dtype=dtype, requires_grad=want_llr)
    J, per_iter, post = forward(g, x, bt, beta_slot, at, alpha_slot, T, targets, weights, offset, dtype)
    wrt = (bt, at, x) if want_llr else (bt, at)
    grads = torch.autograd.grad(J, wrt, allow_unused=True)
    grads = [torch.zeros_like(v) if gr is None else gr for gr, v in zip(grads, wrt)]
    out = {"loss": float(J.detach()), "loss_per_iter": np.array([float(v.detach()) for v in per_iter]),
           "grad_beta": grads[0].numpy(), "grad_alpha": grads[1].numpy(), "posterior": post.detach().numpy()}
    if want_llr:
        out["grad_llr"] = grads[2].numpy()
    return out
