"""
CPU restatement of posterior joint training under the layered schedule (ldpc_train_joint_layered, include/ldpc_hip.h)
-- the yardstick of tests/test_layered_joint_training_host.py and tests/test_gpu_layered_joint_training.py.  Nothing in
the reference executes the schedule, let alone a gradient of it.

Two steps.

``walk``   the fixed-T layered decode in fp32 numpy, exactly as tests/layered_minsum_reference.py defines it (every step
           one rounded fp32 operation, no early stop), additionally recording for every iteration t the value
           ``U_t[b, e] = P_v - R_e`` each check update consumed and the posterior ``P_t`` after the iteration's last check.

``forward`` the loss and its layered posterior-local gradient in float64 torch, teacher-forced on those records: for
           each t the edge values are ``u = U_t`` with ``d u_e / d llr_v = 1`` (``u_e = llr_v + x_e``, x_e a constant), the
           messages ``r`` come from a check update written with the torch operations -- and therefore the tie rules -- of
           the differentiable oracle's check update (oracle/grad_oracle.py: ``min(dim)`` sends the minimum's gradient to
           the first arg-min edge, ``amin`` splits the second minimum's evenly over the edges tied for it, ``sign(0) = 0``,
           ``relu'(0) = 0``, degree 1: ``min2 = min1``; the sign product, which has no gradient, is formed from counts), and
           the posterior is ``l = P_t.detach() + (s - s.detach())`` with
           ``s = llr + scatter_add(r)``: the recorded value, the gradient of "LLR plus this iteration's messages".
           ``J_t = mean BCEWithLogits(-l, y)``, ``J = sum_t w_t J_t``; autograd does the rest.

``closed_form`` is the same gradient written a third time with no autograd at all: scalar loops over codewords, checks and
edges with the derivative formulas of include/ldpc_hip.h spelt out, on its own scalar fp32 walk (the order of operations of
``layered_minsum_reference.restate_scalar``), the gradient sums in float64.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

import layered_minsum_reference as ref

F = np.float32


def walk(graph, llr, T, form, beta_e, a_e=None):
    """``ref.restate(early_stop=False)`` with records -> (U fp32 [T, B, E], P fp32 [T, B, n]); P[T-1] is the decode's
    posterior"""
    assert form in (ref.NMS, ref.OMS)
    P = np.array(llr, dtype=F, copy=True)
    B = P.shape[0]
    R = np.zeros((B, graph.E), dtype=F)
    beta_e = np.asarray(beta_e, dtype=F)
    a_e = None if a_e is None else np.asarray(a_e, dtype=F)
    U = np.zeros((T, B, graph.E), dtype=F)
    Ps = np.zeros((T, B, graph.n), dtype=F)
    cp, vi = graph.check_ptr, graph.var_idx
    ar = np.arange(B)
    for t in range(T):
        for i in range(graph.m):
            e0, e1 = int(cp[i]), int(cp[i + 1])
            dc = e1 - e0
            if dc == 0:
                continue
            V = vi[e0:e1]
            u = P[:, V] - R[:, e0:e1]
            sg = np.sign(u).astype(F)
            mg = np.abs(u)
            k = np.argmin(mg, axis=1)
            m1 = mg[ar, k]
            if dc > 1:
                other = mg.copy()
                other[ar, k] = np.inf
                m2 = other.min(axis=1)
            else:
                m2 = m1
            zeros = (sg == 0).sum(axis=1, keepdims=True) - (sg == 0)
            negs = (sg < 0).sum(axis=1, keepdims=True) - (sg < 0)
            prod = np.where(zeros > 0, F(0), np.where(negs % 2 == 1, F(-1), F(1))).astype(F)
            raw = np.where(np.arange(dc)[None, :] == k[:, None], m2[:, None], m1[:, None]).astype(F)
            b = beta_e[t, e0:e1][None, :]
            if form == ref.NMS:
                r = (b * raw) * prod
            else:
                d = raw - b
                relu = np.where(d > 0, d, F(0)).astype(F)
                a = F(0) if a_e is None else a_e[t, e0:e1][None, :]
                r = prod * (relu - a)
            r = r.astype(F)
            U[t, :, e0:e1] = u
            P[:, V] = u + r
            R[:, e0:e1] = r
        Ps[t] = P
    return U, Ps


def _neighbourhoods(graph):
    """check -> its CSR edges, padded with E: [m, max_dc]"""
    cp = np.asarray(graph.check_ptr, dtype=np.int64)
    dc = np.diff(cp)
    ce = np.full((graph.m, max(int(dc.max()) if graph.m else 1, 1)), graph.E, dtype=np.int64)
    for i in range(graph.m):
        ce[i, :dc[i]] = np.arange(cp[i], cp[i + 1])
    return torch.from_numpy(ce), torch.from_numpy(dc), torch.from_numpy(cp)


def check_update(graph, u, beta_e, a_e, offset):
    """messages r [B, E] of one pass over ALL checks given every edge's consumed value u [B, E] (float64, differentiable);
    beta_e [E], a_e [E] | None: this iteration's weight of every edge.  The operations of oracle/grad_oracle.py:79-102."""
    dtype = u.dtype
    B, E = u.shape
    ce, dc, cp = _neighbourhoods(graph)
    cmask = ce < E
    max_dc = ce.shape[1]
    chk_of_edge = torch.repeat_interleave(torch.arange(graph.m), dc)
    pos_of_edge = torch.arange(E) - cp[chk_of_edge]
    inf = torch.tensor(float("inf"), dtype=dtype)
    pad = torch.cat([u, torch.zeros(B, 1, dtype=dtype)], dim=1)
    inc = pad[:, ce]                                                       # [B, m, max_dc]
    mags = torch.where(cmask, inc.abs(), inf)
    signs = torch.where(cmask, torch.sign(inc), torch.ones((), dtype=dtype))
    m1, i1 = mags.min(dim=-1, keepdim=True)                               # gradient to the (first) arg-min edge
    m2 = mags.scatter(-1, i1, float("inf")).amin(dim=-1, keepdim=True)    # gradient split evenly over the ties
    m2 = torch.where((dc == 1).view(1, -1, 1), m1, m2)
    pos = torch.arange(max_dc).view(1, 1, -1)
    minval = torch.where(pos == i1, m2, m1)
    # product of the OTHER signs, sign(0) = 0.  It carries no gradient (d sign = 0), so it is formed from counts -- the
    # oracle's [.., max_dc, max_dc] product would not fit for the 129-edge check of the wide code
    zero, neg = (signs == 0), (signs < 0)
    zeros_others = zero.sum(dim=-1, keepdim=True) - zero.to(torch.int64)
    negs_others = neg.sum(dim=-1, keepdim=True) - neg.to(torch.int64)
    prod_others = torch.where(zeros_others > 0, torch.zeros((), dtype=dtype),
                              torch.where(negs_others % 2 == 1, -torch.ones((), dtype=dtype), torch.ones((), dtype=dtype)))
    raw = minval[:, chk_of_edge, pos_of_edge]                              # back to CSR edge order
    prod = prod_others[:, chk_of_edge, pos_of_edge]
    if offset:
        a = torch.zeros((), dtype=dtype) if a_e is None else a_e.view(1, -1)
        return prod * (torch.relu(raw - beta_e.view(1, -1)) - a)
    return beta_e.view(1, -1) * (raw * prod)


def forward(graph, llr, U, P, beta_table, beta_slot, oms_table=None, oms_slot=None, offset=False, targets=None,
            weights=None):
    """llr [B, n] torch (float64 leaf when d J/d llr is wanted); U [T, B, E], P [T, B, n] from ``walk``; beta_table [T, Sb]
    and (offset form) oms_table [T, So] | None: torch tables that may require grad, *_slot [E] the column of every edge.
    -> (J, [J_t])  -- call ``J.backward()`` or ``torch.autograd.grad``"""
    T = U.shape[0]
    dtype = torch.float64
    x = llr.to(dtype)
    B, n = x.shape
    voe = torch.from_numpy(np.asarray(graph.var_idx, dtype=np.int64))
    bslot = torch.from_numpy(np.asarray(beta_slot, dtype=np.int64))
    oslot = None if oms_table is None else torch.from_numpy(np.asarray(oms_slot, dtype=np.int64))
    y = torch.zeros((B, n), dtype=dtype) if targets is None else torch.as_tensor(targets).to(dtype)
    w = torch.full((T,), 1.0 / T, dtype=dtype) if weights is None else torch.as_tensor(weights).to(dtype)
    xe = x[:, voe]
    per, J = [], torch.zeros((), dtype=dtype)
    for t in range(T):
        # u = llr_v + (U_t - llr_v).detach(), written so that the VALUE is the recorded fp32 number exactly
        u = torch.from_numpy(U[t]).to(dtype) + (xe - xe.detach())
        r = check_update(graph, u, beta_table[t].to(dtype)[bslot],
                         None if oms_table is None else oms_table[t].to(dtype)[oslot], offset)
        s = x + torch.zeros((B, n), dtype=dtype).index_add(1, voe, r)
        lt = torch.from_numpy(P[t]).to(dtype) + (s - s.detach())
        Jt = Fn.binary_cross_entropy_with_logits(-lt, y)
        per.append(Jt)
        J = J + w[t] * Jt
    return J, per


def closed_form(graph, llr, T, form, beta_e, a_e=None, targets=None, weights=None):
    """the definition of include/ldpc_hip.h with no autograd: a scalar fp32 walk per codeword (each step one rounded
    operation, so ties and zeros fall where the decode has them) and the derivative formulas written out in float64.  -> dict(per_iter [T], grad_beta_e [T, E], grad_a_e [T, E], grad_llr [B, n], posterior [B, n])"""
    llr = np.asarray(llr, dtype=F)
    B, n = llr.shape
    E = graph.E
    cp, vi = [int(v) for v in graph.check_ptr], [int(v) for v in graph.var_idx]
    beta_e = np.asarray(beta_e, dtype=F)
    a_e = np.zeros((T, E), dtype=F) if a_e is None else np.asarray(a_e, dtype=F)
    y = np.zeros((B, n)) if targets is None else np.asarray(targets, dtype=np.float64)
    w = np.full(T, 1.0 / T) if weights is None else np.asarray(weights, dtype=np.float64)
    sgn = lambda v: 1.0 if v > 0 else (-1.0 if v < 0 else 0.0)
    per = np.zeros(T)
    gb, ga, gx, post = np.zeros((T, E)), np.zeros((T, E)), np.zeros((B, n)), np.zeros((B, n))
    for b in range(B):
        P, R = llr[b].copy(), np.zeros(E, dtype=F)
        for t in range(T):
            rec = []                                        # per check: (e0, u, raw, prod, arg-min, tied set, m-values)
            for i in range(graph.m):
                e0, dc = cp[i], cp[i + 1] - cp[i]
                if dc == 0:
                    continue
                u = [F(P[vi[e0 + j]] - R[e0 + j]) for j in range(dc)]
                mg = [F(abs(v)) for v in u]
                k = min(range(dc), key=lambda j: (mg[j], j))                    # first arg-min
                m1 = mg[k]
                m2 = m1 if dc == 1 else min(mg[j] for j in range(dc) if j != k)
                tied = [k] if dc == 1 else [j for j in range(dc) if j != k and mg[j] == m2]
                raw = [m2 if j == k else m1 for j in range(dc)]
                prod = [float(np.prod([sgn(u[q]) for q in range(dc) if q != j])) if dc > 1 else 1.0 for j in range(dc)]
                for j in range(dc):
                    e = e0 + j
                    if form == ref.NMS:
                        r = F(F(beta_e[t, e] * raw[j]) * F(prod[j]))
                    else:
                        d = F(raw[j] - beta_e[t, e])
                        r = F(F(prod[j]) * F((d if d > 0 else F(0)) - a_e[t, e]))
                    P[vi[e]] = F(u[j] + r)
                    R[e] = r
                rec.append((e0, u, raw, prod, k, tied))
            # J_t and its seed on the posterior after the last check
            Pd = P.astype(np.float64)
            per[t] += float(np.sum(np.maximum(-Pd, 0) + Pd * y[b] + np.log1p(np.exp(-np.abs(Pd))))) / (B * n)
            g = w[t] * (y[b] - 1.0 / (1.0 + np.exp(Pd))) / (B * n)              # sigmoid(-P) = 1 / (1 + e^P)
            gx[b] += g
            for e0, u, raw, prod, k, tied in rec:
                dc = len(u)
                acc1 = acc2 = 0.0                              # d J_t/d m1, d J_t/d m2
                for j in range(dc):
                    e = e0 + j
                    ge = g[vi[e]]
                    if form == ref.NMS:
                        gb[t, e] += ge * float(raw[j]) * prod[j]
                        gm = ge * float(beta_e[t, e]) * prod[j]
                    else:
                        is_open = 1.0 if F(raw[j] - beta_e[t, e]) > 0 else 0.0
                        gb[t, e] += -ge * prod[j] * is_open
                        ga[t, e] += -ge * prod[j]
                        gm = ge * prod[j] * is_open
                    if j == k:
                        acc2 += gm
                    else:
                        acc1 += gm
                for j in range(dc):
                    gu = (acc1 if j == k else 0.0) + (acc2 / len(tied) if j in tied else 0.0)
                    gx[b, vi[e0 + j]] += gu * sgn(u[j])
        post[b] = P
    return {"per_iter": per, "grad_beta_e": gb, "grad_a_e": ga, "grad_llr": gx, "posterior": post}
