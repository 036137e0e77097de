"""
CPU restatements of the LEVEL gradient of the quantised posterior joint loss (learned quantisers: ldpc_train_joint_ste_levels,
ldpc_train_joint_layered_ste_levels, ``WeightedRCQDecoder(learn_quantizer=True)``), each written twice:

``forward`` / ``layered_forward``   tests/pjt_rcq_reference.forward and tests/layered_pjt_rcq_reference.forward with the
        reconstruction values as a LEAF: ``levels`` [T, L], row t the table of iteration t's quantiser, and
            c2v = deq + mask * (m - m.detach()),   deq = s(code) * levels[t][code mod L]   NOT detached.
        The thresholds as decision boundaries stay constants (the codes are the recorded ones; the restatement's own
        quantiser, kept for the disagreement share, compares against the detached values), and so do the leave-one-out sums
        of the next variable update.  torch autograd gives d J / d levels [T, L].
``closed_form`` / ``layered_closed_form``   the definition of include/ldpc_hip.h in numpy float64, no autograd:
            grad_levels[t][l] = sum over b, e of [code_t[b, e] mod L == l] * s(code_t[b, e]) * g_t[b, var(e)],
            g_t = w_t * (y - sigmoid(-l_t)) / (B n),  l_t = llr + the reconstructed codes at the variable (flooding),
            l_t = P_t of the walk (layered).

``param_grads`` carries a [T, L] table to ``(C, gamma)`` by torch autograd through tau_j = C * x_j^gamma in float64, the
gamma term taken on 1 <= j <= L - 2 only.  Test infrastructure, not product code.
"""
import numpy as np
import torch
import torch.nn.functional as F

import layered_pjt_reference as lpjt
import pjt_rcq_reference as flood
from grad_oracle import _padded_neighbourhoods


def level_rows(thresholds, q_of_iter, T, dtype=torch.float32):
    """the leaf: [T, L], row t = the table of the quantiser of iteration t"""
    thr = np.asarray(thresholds, dtype=np.float32)
    return torch.tensor(thr[np.asarray(q_of_iter[:T], dtype=np.int64)], dtype=dtype, requires_grad=True)


def forward(g, llr, codes, beta_table, beta_slot, alpha_table, alpha_slot, levels, T, targets=None, weights=None,
            dtype=torch.float32):
    """pjt_rcq_reference.forward with `levels` [T, L] (torch, may require grad) in the place of thresholds / q_of_iter
    -> (J, [J_t], final posterior, disagreement share)"""
    B, n = llr.shape
    E = g.E
    L = levels.shape[1]
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
    per_iter, post, differ = [], llr, 0
    for t in range(T):
        tau = levels[t].to(dtype)
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
        code = codes[:, t, :]
        level = code % L
        deq = (1.0 - 2.0 * (code >= L).to(dtype)) * tau[level]              # the leaf: NOT detached
        mask = (level < L - 1).to(dtype)
        c2v = deq + mask * (m - m.detach())
        md, taud = m.detach(), tau.detach()                                   # the boundaries: constants
        own = torch.zeros_like(code)
        for q in range(L):
            own = torch.where(md.abs() >= taud[q], torch.full_like(own, q), own)
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


def _seed(l, y, w_t):
    """g = w_t * (y - sigmoid(-l)) / (B n), float64"""
    B, n = l.shape
    return w_t * (y - 1.0 / (1.0 + np.exp(l))) / (B * n)


def _level_sums(codes_t, g_t, var_idx, L):
    """[B, E] codes and [B, n] seed of one iteration -> [L] float64"""
    codes_t = np.asarray(codes_t, dtype=np.int64)
    lvl, sgn = codes_t % L, np.where(codes_t >= L, -1.0, 1.0)
    ge = sgn * g_t[:, np.asarray(var_idx, dtype=np.int64)]
    return np.array([ge[lvl == l].sum() for l in range(L)], dtype=np.float64)


def closed_form(g, llr, codes, thresholds, q_of_iter, T, targets=None, weights=None):
    """flooding.  codes uint8 [B, T, E] of the fixed-T decode -> grad_levels float64 [T, L], seeds g_t float64 [T, B, n]"""
    llr = np.asarray(llr, dtype=np.float64)
    B, n = llr.shape
    thr = np.asarray(thresholds, dtype=np.float32).astype(np.float64)
    L = thr.shape[1]
    y = np.zeros((B, n)) if targets is None else np.asarray(targets, dtype=np.float64)
    w = np.full(T, 1.0 / T) if weights is None else np.asarray(weights, dtype=np.float64)
    vi = np.asarray(g.var_idx, dtype=np.int64)
    out, seeds = np.zeros((T, L)), np.zeros((T, B, n))
    for t in range(T):
        c = np.asarray(codes[:, t, :], dtype=np.int64)
        deq = np.where(c >= L, -1.0, 1.0) * thr[int(q_of_iter[t])][c % L]
        l = llr.copy()
        np.add.at(l, (slice(None), vi), deq)
        seeds[t] = _seed(l, y, w[t])
        out[t] = _level_sums(c, seeds[t], vi, L)
    return out, seeds


def layered_forward(graph, llr, U, K, P, beta_table, beta_slot, levels, targets=None, weights=None):
    """layered_pjt_rcq_reference.forward with `levels` [T, L] float64 (torch, may require grad) as the reconstruction values
    -> (J, [J_t])"""
    T = U.shape[0]
    dtype = torch.float64
    x = llr.to(dtype)
    B, n = x.shape
    L = levels.shape[1]
    voe = torch.from_numpy(np.asarray(graph.var_idx, dtype=np.int64))
    bslot = torch.from_numpy(np.asarray(beta_slot, dtype=np.int64))
    y = torch.zeros((B, n), dtype=dtype) if targets is None else torch.as_tensor(targets).to(dtype)
    w = torch.full((T,), 1.0 / T, dtype=dtype) if weights is None else torch.as_tensor(weights).to(dtype)
    xe = x[:, voe]
    per, J = [], torch.zeros((), dtype=dtype)
    for t in range(T):
        u = torch.from_numpy(U[t]).to(dtype) + (xe - xe.detach())
        m = lpjt.check_update(graph, u, beta_table[t].to(dtype)[bslot], None, False)
        code = torch.from_numpy(K[t].astype(np.int64))
        level = code % L
        deq = (1.0 - 2.0 * (code >= L).to(dtype)) * levels[t].to(dtype)[level]     # the leaf: NOT detached
        mask = (level < L - 1).to(dtype)
        r = deq + mask * (m - m.detach())
        s = x + torch.zeros((B, n), dtype=dtype).index_add(1, voe, r)
        lt = torch.from_numpy(P[t]).to(dtype) + (s - s.detach())
        Jt = F.binary_cross_entropy_with_logits(-lt, y)
        per.append(Jt)
        J = J + w[t] * Jt
    return J, per


def layered_closed_form(graph, K, P, L, targets=None, weights=None):
    """layered.  K uint8 [T, B, E] and P fp32 [T, B, n] of the walk -> grad_levels float64 [T, L], seeds [T, B, n]"""
    T, B, n = P.shape
    y = np.zeros((B, n)) if targets is None else np.asarray(targets, dtype=np.float64)
    w = np.full(T, 1.0 / T) if weights is None else np.asarray(weights, dtype=np.float64)
    out, seeds = np.zeros((T, L)), np.zeros((T, B, n))
    for t in range(T):
        seeds[t] = _seed(P[t].astype(np.float64), y, w[t])
        out[t] = _level_sums(K[t], seeds[t], graph.var_idx, L)
    return out, seeds


def per_quantizer(table, q_of_iter, Q):
    """[T, L] rows -> [Q, L]: the rows of every quantiser summed"""
    table = np.asarray(table, dtype=np.float64)
    out = np.zeros((Q, table.shape[1]))
    for t in range(table.shape[0]):
        out[int(q_of_iter[t])] += table[t]
    return out


def param_grads(C, gamma, table_q):
    """d J/d tau [Q, L] -> (d J/d C [Q], d J/d gamma [Q]) by torch autograd through tau_j = C * x_j^gamma in float64;
    the gamma term on 1 <= j <= L - 2 only (tau_0 = C * 0^gamma and tau_L-1 = C enter as functions of C)"""
    C = torch.tensor(np.asarray(C, dtype=np.float64), requires_grad=True)
    gamma = torch.tensor(np.asarray(gamma, dtype=np.float64), requires_grad=True)
    g = torch.as_tensor(np.asarray(table_q, dtype=np.float64))
    L = g.shape[1]
    x = torch.arange(L, dtype=torch.float64) / (L - 1)
    first = C * (x[0] ** gamma.detach())                                          # 0^gamma: 1 at gamma = 0, else 0
    mid = C[:, None] * x[1:L - 1][None, :] ** gamma[:, None]
    tau = torch.cat([first[:, None], mid, C[:, None]], dim=1)
    (tau * g).sum().backward()
    gg = gamma.grad if gamma.grad is not None else torch.zeros_like(gamma)
    return C.grad.numpy(), gg.numpy()


# ---------------------------------------------------------------------------------------------------- per-case results
_FLOOD, _LAYERED = {}, {}


def learnable(plain, **kw):
    """a learn_quantizer decoder with the quantiser parameters and the weights of `plain`"""
    from rcq_decoder import WeightedRCQDecoder
    qp = [(q.C, q.gamma) for q in plain.quantizers]
    dec = WeightedRCQDecoder(plain.code, plain.bc, plain.bv, qp, plain.weight_sharing_type, plain.max_iterations,
                             plain.layered, quantizer_gradient="straight_through",
                             layered_gradient="posterior_local" if plain.layered == "paper" else None,
                             learn_quantizer=True, **kw)
    missing, unexpected = dec.load_state_dict(plain.state_dict(), strict=False)
    assert sorted(missing) == ["quantizer_C", "quantizer_gamma"] and not unexpected
    return dec


def flooding_expected(case):
    """pjt_rcq_cases.CASES[case] -> dict(levels_closed [T, L], levels_autograd [T, L], disagree, seeds, codes, trace_bits,
    trace_posterior), computed once per process, arrays read-only"""
    if case in _FLOOD:
        return _FLOOD[case]
    import pjt_rcq_cases as cases
    _, llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case)
    T = int(dec.max_iterations)
    g = cases.oracle_graph(dec.code)
    lay = dec._sharing_layout()
    thr, qoi = cases.quantiser_tables(dec)
    beta, alpha = dec.weight_tables()
    bits, post, codes = flood.trace(g, llr, beta, lay.beta_slot, alpha, lay.alpha_slot, thr, qoi, T)
    levels = level_rows(thr, qoi, T)
    x = torch.from_numpy(np.asarray(llr, np.float32))
    J, _, _, disagree = forward(g, x, codes, torch.from_numpy(beta), lay.beta_slot, torch.from_numpy(alpha), lay.alpha_slot,
                                levels, T, y, w)
    J.backward()
    closed, seeds = closed_form(g, llr, codes, thr, qoi, T, None if y is None else y.numpy(), None if w is None else w.numpy())
    out = {"levels_closed": closed, "levels_autograd": levels.grad.double().numpy(), "disagree": disagree, "seeds": seeds,
           "codes": codes, "trace_bits": bits, "trace_posterior": post, "q_of_iter": np.asarray(qoi[:T]), "thr": thr}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _FLOOD[case] = out
    return out


def layered_expected(case):
    """layered_pjt_rcq_cases.CASES[case] -> dict(levels_closed, levels_autograd, seeds, q_of_iter, thr), once per process"""
    if case in _LAYERED:
        return _LAYERED[case]
    import layered_pjt_rcq_cases as cases
    _, llr, y, w = cases.inputs(case)
    dec = cases.decoder_of(case)
    T = int(dec.max_iterations)
    graph = dec.code.tanner_graph()
    lay = dec._sharing_layout()
    thr, qoi = cases.quantiser_tables(dec)
    U, K, P = cases.walk_of(dec, llr)
    levels = level_rows(thr, qoi, T, torch.float64)
    beta, _ = dec.weight_tables()
    x = torch.from_numpy(np.asarray(llr, np.float64))
    J, _ = layered_forward(graph, x, U, K, P, torch.from_numpy(beta).double(), lay.beta_slot, levels, y, w)
    J.backward()
    closed, seeds = layered_closed_form(graph, K, P, thr.shape[1], None if y is None else y.numpy(),
                                        None if w is None else w.numpy())
    out = {"levels_closed": closed, "levels_autograd": levels.grad.numpy(), "seeds": seeds, "K": K, "P": P,
           "q_of_iter": np.asarray(qoi[:T]), "thr": thr}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _LAYERED[case] = out
    return out
