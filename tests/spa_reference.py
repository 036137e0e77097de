"""
numpy restatement of the sum-product decoder (LDPC_C2V_SPA, include/ldpc_hip.h).  Not a test module;
tests/test_sum_product_host.py and tests/test_gpu_sum_product.py import it.

Flooding schedule.  x_e is the variable-to-check message on edge e (the LLR of its variable in iteration 0).  On the
edges 0 .. dc-1 of a check, in CSR order:

    g(x)    = log1p(exp(-x))
    a [+] b = sign(a) sign(b) min(|a|, |b|) + (g(|a + b|) - g(|a - b|))       (= 2 atanh(tanh(a/2) tanh(b/2)))
    f_k = f_k-1 [+] x_k,  b_k = x_k [+] b_k+1,  c2v_k = scale * (f_k-1 [+] b_k+1),  c2v_0 = scale * b_1,  c2v_dc-1 = scale * f_dc-2

The sign is the sign BIT (so -0.0 counts as negative; with a zero magnitude the value is 0 either way) and the correction is
one difference that is then added: the operation is exactly odd in each argument and exactly commutative.  The variable
side is that of the normalised min-sum decoder: posterior = llr + sum of the variable's messages, v2c = llr + alpha * sum of
the OTHER messages (sums left to right in ascending check order), decision posterior < 0, syndrome on the decisions, and
with early stop a codeword's outputs are those of the first iteration whose syndrome is zero (iterations 1-based, success),
else of iteration T (no success) -- the stop rule of ldpc_decode.

Every operation is rounded in `dtype` (float32, float64 or longdouble); checks of one degree are processed together and
codewords are a leading axis, so a whole batch is restated at once.
"""
import numpy as np


def boxplus(a, b):
    """a [+] b elementwise, every operation in the arrays' dtype"""
    a, b = np.asarray(a), np.asarray(b)
    with np.errstate(over="ignore", under="ignore"):   # |a + b| may round to inf (g = 0), exp(-x) to a subnormal or 0
        m = np.minimum(np.abs(a), np.abs(b))
        sm = np.where(np.signbit(a) ^ np.signbit(b), -m, m)
        gp = np.log1p(np.exp(-np.abs(a + b)))
        gm = np.log1p(np.exp(-np.abs(a - b)))
        return sm + (gp - gm)


def check_update(x, scale=1.0):
    """x [..., dc] incoming messages of checks of ONE degree dc >= 2 -> c2v [..., dc]"""
    x = np.asarray(x)
    dc = x.shape[-1]
    if dc < 2:
        raise ValueError("the sum-product message of a degree-1 check is infinite")
    dt = x.dtype
    pre = [None] * dc            # pre[k] = x_0 [+] .. [+] x_k-1   (k >= 1)
    pre[1] = x[..., 0]
    for k in range(2, dc):
        pre[k] = boxplus(pre[k - 1], x[..., k - 1])
    out = np.empty_like(x)
    suf = None                   # x_k+1 [+] .. [+] x_dc-1
    for k in range(dc - 1, -1, -1):
        if k == dc - 1:
            msg = pre[k]
        elif k == 0:
            msg = suf
        else:
            msg = boxplus(pre[k], suf)
        out[..., k] = dt.type(scale) * msg
        if k > 0:
            suf = x[..., k] if k == dc - 1 else boxplus(x[..., k], suf)
    return out


class Graph:
    """CSR edge list + what the restatement needs of it (checks grouped by degree, CSC lists)"""

    def __init__(self, n, check_ptr, var_idx):
        self.n = int(n)
        self.check_ptr = np.asarray(check_ptr, dtype=np.int64)
        self.var_idx = np.asarray(var_idx, dtype=np.int64)
        self.m = self.check_ptr.size - 1
        self.E = int(self.var_idx.size)
        self.dc = np.diff(self.check_ptr)
        self.groups = []         # (edge ids [n_checks, dc]) per degree >= 2
        for d in np.unique(self.dc):
            if d == 0:
                continue
            if d == 1:
                raise ValueError("the sum-product decoder refuses a graph with a degree-1 check")
            rows = np.nonzero(self.dc == d)[0]
            self.groups.append(self.check_ptr[rows][:, None] + np.arange(d)[None, :])
        self.check_of_edge = np.repeat(np.arange(self.m), self.dc)
        order = np.argsort(self.var_idx, kind="stable")          # CSC: ascending check inside a variable
        self.var_edges = [[] for _ in range(self.n)]
        for e in order:
            self.var_edges[self.var_idx[e]].append(int(e))
        self.dv = np.array([len(v) for v in self.var_edges], dtype=np.int64)
        # padded CSC table for vectorised sums: [n, max_dv] edge ids, -1 = none
        mdv = int(self.dv.max()) if self.n else 0
        self.csc = -np.ones((self.n, max(mdv, 1)), dtype=np.int64)
        for j, v in enumerate(self.var_edges):
            self.csc[j, :len(v)] = v

    @classmethod
    def of(cls, g):
        """from a TannerGraph (or anything with n, check_ptr, var_idx)"""
        return cls(g.n, g.check_ptr, g.var_idx)

    def unsat(self, bits):
        """[B] bool: some check of the codeword is violated"""
        contrib = np.asarray(bits, dtype=np.int64)[:, self.var_idx]
        cs = np.concatenate([np.zeros((contrib.shape[0], 1), np.int64), np.cumsum(contrib, axis=1)], axis=1)
        par = (cs[:, self.check_ptr[1:]] - cs[:, self.check_ptr[:-1]]) & 1
        return par.any(axis=1)


def check_sweep(graph, x_edges, scale=1.0):
    """x_edges [B, E] -> c2v [B, E] (degree-0 checks have no edge)"""
    out = np.zeros_like(x_edges)
    for ids in graph.groups:
        out[:, ids] = check_update(x_edges[:, ids], scale)
    return out


def variable_sweep(graph, llr, c2v, alpha=1.0):
    """-> (posterior [B, n], v2c [B, E]); sums left to right in CSC order, rounded in the dtype"""
    dt = llr.dtype
    B = llr.shape[0]
    total = np.zeros((B, graph.n), dtype=dt)
    v2c = np.zeros((B, graph.E), dtype=dt)
    mdv = graph.csc.shape[1]
    cols = [np.where((graph.csc[:, k] >= 0)[None, :], c2v[:, np.maximum(graph.csc[:, k], 0)], dt.type(0)) for k in range(mdv)]
    for k in range(mdv):
        total = total + cols[k]
    for skip in range(mdv):
        has = graph.csc[:, skip] >= 0
        if not has.any():
            continue
        s = np.zeros((B, graph.n), dtype=dt)
        for k in range(mdv):
            if k != skip:
                s = s + cols[k]
        val = llr + dt.type(alpha) * s
        v2c[:, graph.csc[has, skip]] = val[:, has]
    return llr + total, v2c


def decode(graph, llr, T, dtype=np.float64, scale=1.0, alpha=1.0):
    """Restate T iterations (no early stop) and derive the early-stop outputs from them.
    graph: Graph, or an object with n / check_ptr / var_idx;  llr [B, n] (or [n]).
    Returns a dict:
      posterior [T, B, n], c2v [T, B, E]   of every iteration, in `dtype`
      bits [T, B, n] uint8                 posterior < 0
      ok [T, B] bool                       the iteration's syndrome is zero
      stop_iterations [B] int32, stop_success [B] bool, stop_bits [B, n] uint8, stop_posterior [B, n]
                                           ldpc_decode(early_stop = 1): first iteration with a zero syndrome (1-based), else T
    """
    if not isinstance(graph, Graph):
        graph = Graph.of(graph)
    dt = np.dtype(dtype)
    llr = np.atleast_2d(np.asarray(llr)).astype(dt)
    B = llr.shape[0]
    post_all = np.zeros((T, B, graph.n), dtype=dt)
    c2v_all = np.zeros((T, B, graph.E), dtype=dt)
    x = llr[:, graph.var_idx]
    for t in range(T):
        c2v = check_sweep(graph, x, scale)
        post, x = variable_sweep(graph, llr, c2v, alpha)
        post_all[t], c2v_all[t] = post, c2v
    bits = (post_all < 0).astype(np.uint8)
    ok = np.stack([~graph.unsat(bits[t]) for t in range(T)]) if T else np.zeros((0, B), bool)
    stop = np.full(B, T, dtype=np.int32)
    succ = np.zeros(B, dtype=bool)
    for t in range(T - 1, -1, -1):
        stop[ok[t]] = t + 1
        succ |= ok[t]
    if T:
        idx = np.maximum(stop - 1, 0)
        stop_bits = bits[idx, np.arange(B)]
        stop_post = post_all[idx, np.arange(B)]
    else:
        stop_bits = (llr < 0).astype(np.uint8)
        stop_post = llr.copy()
    return {"posterior": post_all, "c2v": c2v_all, "bits": bits, "ok": ok, "stop_iterations": stop,
            "stop_success": succ, "stop_bits": stop_bits, "stop_posterior": stop_post}


def ulp(x, dtype):
    """one unit in the last place of |x| in `dtype` (elementwise; the smallest subnormal at 0)"""
    x = np.abs(np.asarray(x, dtype=dtype))
    return np.nextafter(x, np.asarray(np.inf, dtype=dtype)) - x


def tolerance(lo, hi, value_dtype):
    """The tolerance rule.  lo / hi: one quantity restated in the lower and the higher precision (float32 / float64 for the
    fp32 engine, float64 / longdouble for the fp64 engine).  D = max |lo - hi|; the bound for an engine value compared with
    `hi` is 4 D, but never tighter than one ulp (of value_dtype) of the value.  -> (D, bound array shaped like hi)"""
    hi_l = np.asarray(hi, dtype=np.longdouble)
    D = float(np.max(np.abs(np.asarray(lo, dtype=np.longdouble) - hi_l))) if hi_l.size else 0.0
    bound = np.maximum(np.longdouble(4.0 * D), ulp(hi, value_dtype).astype(np.longdouble))
    return D, bound


def awgn_inputs(n, frames, snr_db, seed=7):
    """the tolerance input sets: default_rng(seed), llr = float32(2 (1 + sigma z) / sigma^2), sigma^2 = 10^(-snr/10)"""
    rng = np.random.default_rng(seed)
    s2 = 10.0 ** (-snr_db / 10.0)
    z = rng.standard_normal((frames, n))
    return (2.0 * (1.0 + np.sqrt(s2) * z) / s2).astype(np.float32)


def non_decisive(lo, hi, T_stop):
    """[B] bool per frame: at some iteration t < its stop iteration (of the `hi` restatement) some |posterior| < 8 D_t,
    D_t = max |lo - hi| over the posterior of iteration t.  -> (flags, D [T])"""
    T, B = hi["posterior"].shape[:2]
    D = np.array([np.max(np.abs(lo["posterior"][t].astype(np.longdouble) - hi["posterior"][t])) for t in range(T)], dtype=np.float64)
    flags = np.zeros(B, dtype=bool)
    for t in range(T):
        live = T_stop > t
        flags |= live & (np.abs(hi["posterior"][t]).min(axis=1) < 8.0 * D[t])
    return flags, D
