"""
CPU restatement of posterior joint training of the quantised decoder under the paper's layered schedule
(``WeightedRCQDecoder(layered="paper")``, ldpc_train_joint_layered_ste, include/ldpc_hip.h) -- the yardstick of
tests/test_layered_joint_training_rcq_host.py and tests/test_gpu_layered_joint_training_rcq.py.  Nothing in the reference
executes the schedule, let alone a gradient of it.

``walk``        the fixed-T paper-schedule decode in fp32 numpy (every step one rounded fp32 operation, no early stop),
                recording for every iteration t the value ``U_t[b, e] = P_v - Q^-1_t'(code_e)`` each check update consumed,
                the code ``K_t[b, e] = (m < 0) * L + level`` it wrote and the posterior ``P_t`` after the iteration's last
                check.  FREE-RUNNING: unlike the flooding restatement (tests/pjt_rcq_reference.py, forced on the oracle's
                codes) this forward has no summation order anywhere, so a scalar restatement gives the decode's own bits and
                its codes are exact.
``forward``     the loss and its gradient in float64 torch, teacher-forced on the walk's own records, written like
                ``layered_pjt_reference.forward``: u = U_t with d u_e / d llr_v = 1, m from the differentiable check update
                (``layered_pjt_reference.check_update``: first-index arg-min, the second minimum's gradient split over its
                ties, sign(0) = 0, degree 1: min2 = min1), the message r = deq.detach() + mask * (m - m.detach()) with the
                reconstruction and the straight-through mask ``K_t mod L < L - 1`` taken from the recorded codes, and the
                posterior l = P_t.detach() + (s - s.detach()), s = llr + scatter_add(r).  It also quantises its own m
                (rounded to fp32: the product of two fp32 numbers in float64 is exact) and returns the share of (b, t, e)
                on which that differs from the recorded code -- 0 unless the two statements disagree.
``closed_form`` the same gradient a third time with no autograd: scalar loops over codewords, checks and edges on its own
                scalar fp32 walk, the derivative formulas of include/ldpc_hip.h written out, sums in float64.
"""
import numpy as np
import torch
import torch.nn.functional as Fn

import layered_pjt_reference as pjt

F = np.float32


def _quantise(m, tau):
    """fp32 m [..], tau fp32 [L] -> (level = last q with |m| >= tau_q (0 when none), negative flag)"""
    mag = np.abs(m)
    lvl = np.zeros(m.shape, dtype=np.int64)
    for q in range(tau.shape[0]):
        lvl = np.where(mag >= tau[q], q, lvl)
    return lvl, m < 0


def walk(graph, llr, T, beta_e, thresholds, q_of_iter):
    """beta_e fp32 [T, E]: beta_t of every CSR edge; thresholds fp32 [Q, L]; q_of_iter [T]
    -> (U fp32 [T, B, E], K uint8 [T, B, E], P fp32 [T, B, n]); P[T-1] is the decode's posterior, K[T-1] its final codes"""
    P = np.array(llr, dtype=F, copy=True)
    B = P.shape[0]
    thr = np.asarray(thresholds, dtype=F)
    L = thr.shape[1]
    beta_e = np.asarray(beta_e, dtype=F)
    R = np.zeros((B, graph.E), dtype=F)              # the reconstruction of every edge's stored code; none in iteration 0
    U = np.zeros((T, B, graph.E), dtype=F)
    K = np.zeros((T, B, graph.E), dtype=np.uint8)
    Ps = np.zeros((T, B, graph.n), dtype=F)
    cp, vi = graph.check_ptr, graph.var_idx
    ar = np.arange(B)
    for t in range(T):
        tau = thr[int(q_of_iter[t])]
        for i in range(graph.m):
            e0, e1 = int(cp[i]), int(cp[i + 1])
            dc = e1 - e0
            if dc == 0:
                continue
            V = vi[e0:e1]
            u = P[:, V] if t == 0 else P[:, V] - R[:, e0:e1]          # iteration 0: nothing is subtracted
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
            m = ((beta_e[t, e0:e1][None, :] * raw).astype(F) * prod).astype(F)   # the product rounded, then the sign
            lvl, neg = _quantise(m, tau)
            r = np.where(neg, -tau[lvl], tau[lvl]).astype(F)
            U[t, :, e0:e1] = u
            K[t, :, e0:e1] = neg * L + lvl
            P[:, V] = (u + r).astype(F)
            R[:, e0:e1] = r
        Ps[t] = P
    return U, K, Ps


def forward(graph, llr, U, K, P, beta_table, beta_slot, thresholds, q_of_iter, targets=None, weights=None):
    """llr [B, n] torch (float64 leaf when d J/d llr is wanted); U, K, P from ``walk``; beta_table [T, Sb] torch (may
    require grad), beta_slot [E].  -> (J, [J_t], share of (b, t, e) where the own quantiser differs from K)"""
    T = U.shape[0]
    dtype = torch.float64
    x = llr.to(dtype)
    B, n = x.shape
    thr = np.asarray(thresholds, dtype=F)
    L = thr.shape[1]
    voe = torch.from_numpy(np.asarray(graph.var_idx, dtype=np.int64))
    bslot = torch.from_numpy(np.asarray(beta_slot, dtype=np.int64))
    y = torch.zeros((B, n), dtype=dtype) if targets is None else torch.as_tensor(targets).to(dtype)
    w = torch.full((T,), 1.0 / T, dtype=dtype) if weights is None else torch.as_tensor(weights).to(dtype)
    xe = x[:, voe]
    per, J, differ = [], torch.zeros((), dtype=dtype), 0
    for t in range(T):
        tau = thr[int(q_of_iter[t])]
        u = torch.from_numpy(U[t]).to(dtype) + (xe - xe.detach())        # the recorded fp32 value exactly
        m = pjt.check_update(graph, u, beta_table[t].to(dtype)[bslot], None, False)
        code = K[t].astype(np.int64)
        level = code % L
        deq = torch.from_numpy(np.where(code >= L, -1.0, 1.0) * tau[level].astype(np.float64))
        mask = torch.from_numpy((level < L - 1).astype(np.float64))
        r = deq + mask * (m - m.detach())
        lvl, neg = _quantise(m.detach().numpy().astype(F), tau)
        differ += int(((neg * L + lvl) != code).sum())
        s = x + torch.zeros((B, n), dtype=dtype).index_add(1, voe, r)
        lt = torch.from_numpy(P[t]).to(dtype) + (s - s.detach())
        Jt = Fn.binary_cross_entropy_with_logits(-lt, y)
        per.append(Jt)
        J = J + w[t] * Jt
    return J, per, differ / max(B * T * graph.E, 1)


def closed_form(graph, llr, T, beta_e, thresholds, q_of_iter, targets=None, weights=None):
    """the definition of include/ldpc_hip.h with no autograd: a scalar fp32 walk per codeword and the derivative formulas
    written out in float64 -> dict(per_iter [T], grad_beta_e [T, E], grad_llr [B, n], posterior [B, n], codes [T, B, E])"""
    llr = np.asarray(llr, dtype=F)
    B, n = llr.shape
    E = graph.E
    thr = np.asarray(thresholds, dtype=F)
    L = thr.shape[1]
    cp, vi = [int(v) for v in graph.check_ptr], [int(v) for v in graph.var_idx]
    beta_e = np.asarray(beta_e, dtype=F)
    y = np.zeros((B, n)) if targets is None else np.asarray(targets, dtype=np.float64)
    w = np.full(T, 1.0 / T) if weights is None else np.asarray(weights, dtype=np.float64)
    sgn = lambda v: 1.0 if v > 0 else (-1.0 if v < 0 else 0.0)
    per = np.zeros(T)
    gb, gx, post = np.zeros((T, E)), np.zeros((B, n)), np.zeros((B, n))
    codes = np.zeros((T, B, E), dtype=np.uint8)
    for b in range(B):
        P, R = llr[b].copy(), np.zeros(E, dtype=F)
        for t in range(T):
            tau = thr[int(q_of_iter[t])]
            rec = []                                        # per check: (e0, u, raw, prod, arg-min, tied set, open flags)
            for i in range(graph.m):
                e0, dc = cp[i], cp[i + 1] - cp[i]
                if dc == 0:
                    continue
                u = [P[vi[e0 + j]] if t == 0 else F(P[vi[e0 + j]] - R[e0 + j]) for j in range(dc)]
                mg = [F(abs(v)) for v in u]
                k = min(range(dc), key=lambda j: (mg[j], j))                    # first arg-min
                m1 = mg[k]
                m2 = m1 if dc == 1 else min(mg[j] for j in range(dc) if j != k)
                tied = [k] if dc == 1 else [j for j in range(dc) if j != k and mg[j] == m2]
                raw = [m2 if j == k else m1 for j in range(dc)]
                prod = [float(np.prod([sgn(u[q]) for q in range(dc) if q != j])) if dc > 1 else 1.0 for j in range(dc)]
                passes = []
                for j in range(dc):
                    e = e0 + j
                    m = F(F(beta_e[t, e] * raw[j]) * F(prod[j]))
                    lvl = 0
                    for q in range(L):
                        if abs(m) >= tau[q]:
                            lvl = q
                    r = F(-tau[lvl]) if m < 0 else tau[lvl]
                    codes[t, b, e] = (L if m < 0 else 0) + lvl
                    passes.append(1.0 if lvl < L - 1 else 0.0)                  # straight-through below the top level
                    P[vi[e]] = F(u[j] + r)
                    R[e] = r
                rec.append((e0, u, raw, prod, k, tied, passes))
            Pd = P.astype(np.float64)
            per[t] += float(np.sum(np.maximum(-Pd, 0) + Pd * y[b] + np.log1p(np.exp(-np.abs(Pd))))) / (B * n)
            g = w[t] * (y[b] - 1.0 / (1.0 + np.exp(Pd))) / (B * n)              # sigmoid(-P) = 1 / (1 + e^P)
            gx[b] += g
            for e0, u, raw, prod, k, tied, passes in rec:
                dc = len(u)
                acc1 = acc2 = 0.0                              # d J_t/d m1, d J_t/d m2
                for j in range(dc):
                    e = e0 + j
                    gk = g[vi[e]] * passes[j] * prod[j]
                    gb[t, e] += gk * float(raw[j])
                    gm = gk * float(beta_e[t, e])
                    if j == k:
                        acc2 += gm
                    else:
                        acc1 += gm
                for j in range(dc):
                    gu = (acc1 if j == k else 0.0) + (acc2 / len(tied) if j in tied else 0.0)
                    gx[b, vi[e0 + j]] += gu * sgn(u[j])
        post[b] = P
    return {"per_iter": per, "grad_beta_e": gb, "grad_llr": gx, "posterior": post, "codes": codes}
