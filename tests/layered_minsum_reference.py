"""
Numpy restatement of the layered schedule of the min-sum decoders (``schedule="layered"``: layered_minsum_lds,
ldpc_layered.hip, and layered_minsum, ldpc_kernels.hip) -- the yardstick of tests/test_layered_minsum_host.py and
tests/test_gpu_layered_minsum.py.  Nothing in the reference executes this schedule.

Per codeword the state is fp32: posteriors ``P[n] = llr`` and a message ``R[e] = +0`` on every edge.  For iteration
t = 0..T-1 the checks are walked in CSR order (degree 0 skipped); on the edges e = (i, v) of check i

    u_e    = P_v - R_e
    m1, m2 = smallest / second smallest |u| (first minimum is the arg-min, ties keep m2 == m1, degree 1: m2 = m1)
    raw_e  = m2 on the arg-min edge, else m1
    prod_e = product of sgn(u) over the OTHER edges, sgn(0) = 0          (oracle/ldpc_oracle_impl.h:77, 121-122)
    NMS:  r_e = (beta_t[e] * raw_e) * prod_e                             (:127)
    OMS:  r_e = prod_e * (relu(raw_e - beta_t[e]) - a_t[e])              (:130-133)
    P_v = u_e + r_e ;  R_e = r_e

Every step is one rounded fp32 operation.  The syndrome is taken on ``P < 0`` after the last check of an iteration; with
early stop a codeword whose syndrome is zero stops (iterations = t + 1, success, P and R frozen); without it the decode
runs exactly T iterations and success is "the final syndrome is zero".

``restate`` is vectorised over the batch, one check at a time; ``restate_scalar`` is the same definition written
independently as a per-codeword loop over scalars.
"""
import numpy as np

NMS, OMS = "nms", "oms"
F = np.float32


def unsat(graph, P):
    """[B] bool: some check of the codeword is unsatisfied by the decisions P < 0"""
    hard = (P < 0).astype(np.int64)
    cp, vi = graph.check_ptr, graph.var_idx
    bad = np.zeros(P.shape[0], dtype=np.int64)
    for i in range(graph.m):
        bad |= hard[:, vi[cp[i]:cp[i + 1]]].sum(axis=1) & 1
    return bad.astype(bool)


def restate(graph, llr, T, form, beta_e, a_e=None, early_stop=True, max_iters=None):
    """graph: TannerGraph (n, m, E, check_ptr, var_idx); llr [B, n]; beta_e [T, E] and a_e [T, E] | None (= 0): the
    weights of every CSR edge; max_iters: run at most that many of the T iterations (an open codeword then reports
    iterations = max_iters, success False).
    -> bits int32 [B, n], P fp32 [B, n], iterations int32 [B], success bool [B], R fp32 [B, E] (every edge's last message)"""
    assert form in (NMS, OMS)
    T_run = T if max_iters is None else min(T, int(max_iters))
    P = np.array(llr, dtype=F, copy=True)
    B = P.shape[0]
    R = np.zeros((B, graph.E), dtype=F)
    beta_e = np.asarray(beta_e, dtype=F)
    a_e = None if a_e is None else np.asarray(a_e, dtype=F)
    open_ = np.ones(B, dtype=bool)
    iters = np.full(B, T_run, dtype=np.int32)
    succ = np.zeros(B, dtype=bool)
    cp, vi = graph.check_ptr, graph.var_idx
    for t in range(T_run):
        rows = np.flatnonzero(open_)
        if rows.size == 0:
            break
        ar = np.arange(rows.size)
        for i in range(graph.m):
            e0, e1 = int(cp[i]), int(cp[i + 1])
            dc = e1 - e0
            if dc == 0:
                continue
            V = vi[e0:e1]
            u = P[np.ix_(rows, V)] - R[rows, e0:e1]
            sg = np.sign(u).astype(F)
            mg = np.abs(u)
            k = np.argmin(mg, axis=1)                         # first minimum
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
            if form == NMS:
                r = (b * raw) * prod
            else:
                d = raw - b
                relu = np.where(d > 0, d, F(0)).astype(F)
                a = F(0) if a_e is None else a_e[t, e0:e1][None, :]
                r = prod * (relu - a)
            r = r.astype(F)
            P[np.ix_(rows, V)] = u + r
            R[rows, e0:e1] = r
        if early_stop:
            done = open_ & ~unsat(graph, P)
            iters[done] = t + 1
            succ[done] = True
            open_ &= ~done
    if not early_stop:
        succ = ~unsat(graph, P)
    return (P < 0).astype(np.int32), P, iters, succ, R


def _sgn(x):
    return F(1) if x > 0 else (F(-1) if x < 0 else F(0))


def restate_scalar(graph, llr, T, form, beta_e, a_e=None, early_stop=True):
    """the same decode, one codeword and one scalar at a time (written on its own: loops in the order of
    oracle/ldpc_oracle_impl.h's check update, nothing shared with ``restate``)"""
    llr = np.asarray(llr, dtype=F)
    B, n = llr.shape
    cp, vi = [int(x) for x in graph.check_ptr], [int(x) for x in graph.var_idx]
    bits = np.zeros((B, n), dtype=np.int32)
    post = np.zeros((B, n), dtype=F)
    iters = np.zeros(B, dtype=np.int32)
    succ = np.zeros(B, dtype=bool)
    msgs = np.zeros((B, graph.E), dtype=F)

    def satisfied(P):
        for i in range(graph.m):
            par = 0
            for e in range(cp[i], cp[i + 1]):
                par ^= 1 if P[vi[e]] < 0 else 0
            if par:
                return False
        return True

    for w in range(B):
        P = [F(x) for x in llr[w]]
        R = [F(0)] * graph.E
        it_done, ok = T, False
        for t in range(T):
            for i in range(graph.m):
                e0, dc = cp[i], cp[i + 1] - cp[i]
                if dc == 0:
                    continue
                u = [F(P[vi[e0 + j]] - R[e0 + j]) for j in range(dc)]
                mg = [F(0) if x == 0 else F(abs(x)) for x in u]
                k = 0
                for j in range(1, dc):
                    if mg[j] < mg[k]:
                        k = j
                m1 = m2 = mg[k]
                if dc > 1:
                    m2 = F(np.inf)
                    for j in range(dc):
                        if j != k and mg[j] < m2:
                            m2 = mg[j]
                for j in range(dc):
                    prod = F(1)
                    for q in range(dc):
                        if q != j:
                            prod = F(prod * _sgn(u[q]))
                    raw = m2 if j == k else m1
                    b = F(beta_e[t][e0 + j])
                    if form == NMS:
                        r = F(F(b * raw) * prod)
                    else:
                        d = F(raw - b)
                        relu = d if d > 0 else F(0)
                        a = F(0) if a_e is None else F(a_e[t][e0 + j])
                        r = F(prod * F(relu - a))
                    P[vi[e0 + j]] = F(u[j] + r)
                    R[e0 + j] = r
            if early_stop and satisfied(P):
                it_done, ok = t + 1, True
                break
        if not early_stop:
            ok = satisfied(P)
        post[w] = P
        bits[w] = [1 if x < 0 else 0 for x in P]
        iters[w], succ[w], msgs[w] = it_done, ok, R
    return bits, post, iters, succ, msgs
