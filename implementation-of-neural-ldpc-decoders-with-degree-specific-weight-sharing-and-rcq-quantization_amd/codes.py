"""
Deterministic sparse LDPC code construction for the benchmark configurations.

The reference holds no usable matrix for the sizes BASELINE.json names: its only
real code is the 4x7 toy of ``create_test_ldpc_code`` (ldpc_decoder.py:274-284)
and ``create_dvbs2_code`` (training_framework.py:379-400) is a *dense random*
9000x16200 matrix (~7.3e7 edges).  SURVEY.md section 8(d) therefore specifies
builder-generated IRA-style codes:

* ``ira_1998_1512``  : n=1998, m=486, variable degrees {8:216, 3:1296, 2:485, 1:1}
* ``dvbs2_like_16200_7200`` : n=16200, m=9000, E=48599, node-perspective degree
  profile of the paper's Table II: VN {8:1800, 3:5400, 2:8999, 1:1},
  CN {4:1441, 5:3239, 6:3600, 7:720}
* ``small_96_48`` : n=96, m=48 test code with variable degrees {1,2,3,8}

* ``qc_1944_972`` : n=1944, m=972 quasi-cyclic, mb=12, nb=24, Z=81, dual-diagonal parity part, check degrees 7 and 8,
  no 4-cycles; its 12 block rows are declared as layers (``generate_qc_code``, seed 1944, ``_QC_SPECS``)

Generated edge lists are committed under ``data/`` so every run (here and on
the GPU box) decodes the very same graph; ``generate_ira_code`` is the script
that made them (``python codes.py`` regenerates and verifies the files).  The quasi-cyclic codes of ``_QC_SPECS`` have no
file under ``data/``: ``generate_qc_code`` takes about two seconds, so ``load_graph`` builds them from their seed, once per
process; the recorded edge list of ``qc_1944_972`` is a test vector (tests/golden/qc_1944_972.npz) that pins the generator.

Layers: ``quasi_cyclic`` builds a QC code from any shift table, ``layered_order`` reorders the checks of any graph into
variable-disjoint layers; both return graphs that carry ``layer_ptr`` (tanner_graph.py), which the block-parallel layered
kernel reads.

Construction: the last ``m`` columns are the IRA staircase (parity column p
touches checks p and p+1; the last one only check m-1).  Information columns
take their edges from a shuffled multiset of check "sockets" sized so every
check ends at its target degree; duplicate sockets inside one column and
4-cycles are repaired by socket swaps.
"""

from __future__ import annotations

import os
from typing import Dict, Optional, Sequence

import numpy as np

from tanner_graph import TannerGraph

_DATA_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")


def generate_ira_code(n: int, m: int, info_degrees: Dict[int, int],
                      check_degrees: Optional[Dict[int, int]] = None,
                      seed: int = 0, max_repair_sweeps: int = 200) -> TannerGraph:
    """Build an IRA-style irregular code.

    info_degrees  {dv: number of information columns with that degree}
    check_degrees {dc: number of checks with that (total) degree}; ``None``
                  spreads the edges as evenly as possible.
    """
    k = n - m
    if sum(info_degrees.values()) != k:
        raise ValueError("info_degrees must cover exactly n-m columns")
    rng = np.random.default_rng(seed)

    # parity staircase
    par_rows = [np.arange(m, dtype=np.int64)]            # p -> check p
    par_cols = [k + np.arange(m, dtype=np.int64)]
    par_rows.append(np.arange(1, m, dtype=np.int64))     # p -> check p+1
    par_cols.append(k + np.arange(m - 1, dtype=np.int64))
    par_deg = np.full(m, 2, dtype=np.int64)
    par_deg[0] = 1

    col_deg = np.concatenate([np.full(cnt, dv, dtype=np.int64)
                              for dv, cnt in sorted(info_degrees.items(), reverse=True)])
    # interleave degrees over the column index range so that degree classes are
    # not contiguous blocks (keeps the VN sweep's gather pattern realistic)
    col_deg = col_deg[rng.permutation(k)]
    e_info = int(col_deg.sum())

    if check_degrees is None:
        total = e_info + int(par_deg.sum())
        base, extra = divmod(total, m)
        target = np.full(m, base, dtype=np.int64)
        target[rng.permutation(m)[:extra]] += 1
    else:
        if sum(check_degrees.values()) != m:
            raise ValueError("check_degrees must cover exactly m checks")
        target = np.concatenate([np.full(cnt, dc, dtype=np.int64)
                                 for dc, cnt in sorted(check_degrees.items())])
        target = target[rng.permutation(m)]
        # check 0 has one staircase edge only: give it the smallest target left so
        # capacities stay positive
    cap = target - par_deg
    if cap.min() < 0 or int(cap.sum()) != e_info:
        raise ValueError(f"degree profiles inconsistent: info edges {e_info}, capacity {int(cap.sum())}")

    sockets = np.repeat(np.arange(m, dtype=np.int64), cap)
    rng.shuffle(sockets)
    col_of_socket = np.repeat(np.arange(k, dtype=np.int64), col_deg)
    col_start = np.zeros(k + 1, dtype=np.int64)
    np.cumsum(col_deg, out=col_start[1:])

    def col_checks(c):
        return sockets[col_start[c]:col_start[c + 1]]

    # check -> set of info columns (for 4-cycle detection)
    def build_members():
        mem = [set() for _ in range(m)]
        for s in range(e_info):
            mem[sockets[s]].add(int(col_of_socket[s]))
        return mem

    def bad_sockets(members):
        """socket positions that are duplicates inside their column, or that
        close a 4-cycle with another information column or the staircase."""
        bad = []
        for c in range(k):
            chk = col_checks(c)
            seen = {}
            for t, i in enumerate(chk):
                i = int(i)
                if i in seen:
                    bad.append(col_start[c] + t)
                seen[i] = t
            # staircase 4-cycle: column touches checks i and i+1 -> shares two
            # checks with parity column i
            sset = set(int(x) for x in chk)
            for t, i in enumerate(chk):
                if int(i) + 1 in sset:
                    bad.append(col_start[c] + t)
            # info-info 4-cycles
            other = {}
            for t, i in enumerate(chk):
                for c2 in members[int(i)]:
                    if c2 == c:
                        continue
                    if c2 in other:
                        bad.append(col_start[c] + t)
                    else:
                        other[c2] = t
        return sorted(set(int(b) for b in bad))

    for sweep in range(max_repair_sweeps):
        members = build_members()
        bad = bad_sockets(members)
        if not bad:
            break
        # swap every offending socket with a uniformly random one
        for s in bad:
            t = int(rng.integers(0, e_info))
            sockets[s], sockets[t] = sockets[t], sockets[s]
    # duplicates are fatal, 4-cycles only undesirable: a final duplicate-only repair
    for _ in range(1000):
        dup = []
        for c in range(k):
            chk = col_checks(c)
            if len(set(int(x) for x in chk)) != len(chk):
                u, idx = np.unique(chk, return_index=True)
                mask = np.ones(len(chk), dtype=bool)
                mask[idx] = False
                dup.extend((col_start[c] + np.nonzero(mask)[0]).tolist())
        if not dup:
            break
        for s in dup:
            t = int(rng.integers(0, e_info))
            sockets[s], sockets[t] = sockets[t], sockets[s]
    else:
        raise RuntimeError("could not remove duplicate edges")

    rows = np.concatenate([sockets] + par_rows)
    cols = np.concatenate([col_of_socket] + par_cols)
    return TannerGraph(n, m, rows, cols)


# ---------------------------------------------------------------------------- named codes
_SPECS = {
    "ira_1998_1512": dict(n=1998, m=486, info_degrees={8: 216, 3: 1296}, check_degrees=None, seed=1998),
    "dvbs2_like_16200_7200": dict(n=16200, m=9000, info_degrees={8: 1800, 3: 5400},
                                  check_degrees={4: 1441, 5: 3239, 6: 3600, 7: 720}, seed=16200),
    "small_96_48": dict(n=96, m=48, info_degrees={8: 8, 3: 40}, check_degrees=None, seed=96),
}


# quasi-cyclic codes (generate_qc_code): ``qc_1944_972`` is mb = 12, nb = 24, Z = 81 -- eight information block columns of
# degree 3 and four of degree 11 beside the dual-diagonal parity part, check degrees 7 and 8; layers = block rows
_QC_SPECS = {
    "qc_1944_972": dict(mb=12, nb=24, Z=81, info_degree_profile={3: 8, 11: 4}, seed=1944),
}


def code_names() -> Sequence[str]:
    return tuple(_SPECS) + tuple(_QC_SPECS)


def _path(name: str) -> str:
    return os.path.join(_DATA_DIR, name + ".npz")


def save_graph(path: str, g: TannerGraph) -> None:
    """A graph that declares layers also stores ``layer_ptr``; one without is written exactly as before."""
    extra = {} if g.layer_ptr is None else {"layer_ptr": np.asarray(g.layer_ptr, dtype=np.int32)}
    np.savez_compressed(path, n=np.int32(g.n), m=np.int32(g.m),
                        check_ptr=g.check_ptr, var_idx=g.var_idx.astype(np.uint16 if g.n <= 65535 else np.int32), **extra)


_QC_CACHE: Dict[str, TannerGraph] = {}


def load_graph(name_or_path: str) -> TannerGraph:
    """Load a committed edge list (``data/<name>.npz``, or any path), with its layers when the file has them; a name of
    ``_QC_SPECS`` is generated from its seed (once per process: later calls return the same graph object)."""
    if name_or_path in _QC_SPECS and not os.path.exists(name_or_path):
        if name_or_path not in _QC_CACHE:
            _QC_CACHE[name_or_path] = generate_qc_code(**_QC_SPECS[name_or_path])
        return _QC_CACHE[name_or_path]
    path = name_or_path if os.path.exists(name_or_path) else _path(name_or_path)
    with np.load(path, allow_pickle=False) as z:
        g = TannerGraph.from_csr(int(z["n"]), z["check_ptr"], z["var_idx"].astype(np.int32))
        return g.with_layers(z["layer_ptr"]) if "layer_ptr" in z.files else g


# ---------------------------------------------------------------------------- quasi-cyclic and layer-ordered codes
def quasi_cyclic(shifts, Z: int) -> TannerGraph:
    """The quasi-cyclic code of a shift matrix: ``shifts`` int [mb, nb], a value < 0 is the Z x Z zero block, a value
    s >= 0 the Z x Z identity shifted by s (row z has its one in column (z + s) mod Z).  Checks are ordered block row by
    block row; the checks of a block row share no variable, so the graph declares them as its layers:
    ``layer_ptr = [0, Z, 2Z, ...]``.  A caller with a standard's shift table (802.11n, 5G NR) passes it here."""
    S = np.asarray(shifts)
    if S.ndim != 2 or not np.issubdtype(S.dtype, np.integer):
        raise ValueError("shifts must be an integer array [mb, nb]")
    Z = int(Z)
    if Z < 1:
        raise ValueError("Z must be >= 1")
    mb, nb = S.shape
    br, bc = np.nonzero(S >= 0)
    z = np.arange(Z, dtype=np.int64)
    rows = (br[:, None] * Z + z[None, :]).ravel()
    cols = (bc[:, None] * Z + (z[None, :] + S[br, bc][:, None].astype(np.int64)) % Z).ravel()
    g = TannerGraph(nb * Z, mb * Z, rows, cols)
    return g.with_layers(np.arange(mb + 1, dtype=np.int64) * Z) if mb else g


def layered_order(graph: TannerGraph, max_layer: Optional[int] = None):
    """Reorder the checks of any graph into layers.  First-fit colouring of the checks in ascending order (a check goes to
    the first layer none of whose checks shares a variable with it and that holds fewer than ``max_layer`` checks, when
    given); the rows are then re-emitted layer by layer, ascending inside a layer.  -> (graph2, perm): ``graph2`` carries
    the layers and its row i is row ``perm[i]`` of ``graph``.

    It is the same code with the same codewords -- encoders, channels and error counters need nothing, and the result of
    a FLOODING decode does not depend on the order of the checks.  It is a DIFFERENT layered decoder: the layered
    schedule walks the checks in order, so another order gives other messages, posteriors and iteration counts."""
    if max_layer is not None and int(max_layer) < 1:
        raise ValueError("max_layer must be >= 1")
    cap = None if max_layer is None else int(max_layer)
    var_layers = [set() for _ in range(graph.n)]
    members = []                                        # layer -> checks, ascending
    first_open = 0                                      # layers below are full
    for i in range(graph.m):
        vs = graph.var_idx[graph.check_ptr[i]:graph.check_ptr[i + 1]]
        taken = set()
        for v in vs:
            taken |= var_layers[int(v)]
        l = first_open
        while l < len(members) and (l in taken or (cap is not None and len(members[l]) >= cap)):
            l += 1
        if l == len(members):
            members.append([])
        members[l].append(i)
        for v in vs:
            var_layers[int(v)].add(l)
        while cap is not None and first_open < len(members) and len(members[first_open]) >= cap:
            first_open += 1
    perm = np.asarray([i for layer in members for i in layer], dtype=np.int64)
    new_row = np.empty(graph.m, dtype=np.int64)
    new_row[perm] = np.arange(graph.m)
    g2 = TannerGraph(graph.n, graph.m, new_row[graph.check_of_edge], graph.var_idx)
    ptr = np.concatenate([[0], np.cumsum([len(layer) for layer in members])]).astype(np.int64)
    return (g2.with_layers(ptr) if graph.m else g2), perm.astype(np.int32)


def generate_qc_code(mb: int, nb: int, Z: int, info_degree_profile: Dict[int, int], seed: int = 0,
                     max_draws: int = 10000) -> TannerGraph:
    """Seeded quasi-cyclic code with a dual-diagonal parity part.  The last mb block columns are the parity part: parity
    block column i sits in block rows i and i + 1 (the last one in row mb - 1 only) at shift 0, so H has full rank.  The
    nb - mb information block columns follow ``info_degree_profile`` {block-column degree: count}, highest degree first;
    a column takes the block rows that hold the fewest entries so far (ties in seeded random order), so the check degrees
    come out even.  The shifts of a column are redrawn until it closes no 4-cycle with the columns before it; the
    finished graph is verified with ``four_cycles() == 0``."""
    kb = nb - mb
    if kb < 1 or mb < 1 or sum(info_degree_profile.values()) != kb:
        raise ValueError("info_degree_profile must cover exactly nb - mb block columns")
    if max(info_degree_profile) > mb or min(info_degree_profile) < 1:
        raise ValueError("a block column's degree must be in 1 .. mb")
    rng = np.random.default_rng(seed)
    S = np.full((mb, nb), -1, dtype=np.int64)
    for i in range(mb):
        S[i, kb + i] = 0
        if i + 1 < mb:
            S[i + 1, kb + i] = 0
    load = (S >= 0).sum(axis=1)

    def closes_cycle(col, done):
        ra = np.flatnonzero(S[:, col] >= 0)
        for b in done:
            common = ra[S[ra, b] >= 0]
            d = (S[common, col] - S[common, b]) % Z
            if np.unique(d).size != d.size:            # two common rows with the same shift difference: a 4-cycle
                return True
        return False

    done = list(range(kb, nb))
    degs = [d for d, cnt in sorted(info_degree_profile.items(), reverse=True) for _ in range(cnt)]
    for col, d in enumerate(degs):
        order = rng.permutation(mb)
        rows = order[np.argsort(load[order], kind="stable")[:d]]
        for _ in range(max_draws):
            S[:, col] = -1
            S[rows, col] = rng.integers(0, Z, size=d)
            if not closes_cycle(col, done):
                break
        else:
            raise RuntimeError(f"no 4-cycle-free shifts for block column {col} at Z = {Z}")
        load[rows] += 1
        done.append(col)
    g = quasi_cyclic(S, Z)
    if g.four_cycles() != 0:
        raise RuntimeError("generated QC code has 4-cycles")
    return g


def load_code(name: str, max_iterations: int = 50):
    """Named code as an ``LDPCCode`` (dense ``H`` materialised lazily as int8)."""
    from ldpc_decoder import LDPCCode
    g = load_graph(name)
    return LDPCCode.from_graph(g, k=g.n - g.m, max_iterations=max_iterations)


def staircase_encode(graph: TannerGraph, info_bits) -> np.ndarray:
    """Systematic encoding on a graph whose last m columns are the IRA staircase (parity column p on checks p and p + 1, the
    last one on check m - 1 only): p_i = p_{i-1} + (H_info u)_i over GF(2).  info_bits: 0/1, [k] or [B, k] with k = n - m
    -> uint8 codewords [n] or [B, n] with H c = 0.  numpy, on the host.  ValueError when the last m columns are not that
    staircase."""
    n, m = graph.n, graph.m
    k = n - m
    rows, cols = np.asarray(graph.check_of_edge, dtype=np.int64), np.asarray(graph.var_idx, dtype=np.int64)
    par = cols >= k
    have = np.unique(rows[par] * m + (cols[par] - k))                                 # (check, parity column) pairs, sorted
    p = np.arange(m, dtype=np.int64)
    want = np.unique(np.concatenate([p * m + p, (p[:-1] + 1) * m + p[:-1]]))
    if k < 1 or int(par.sum()) != want.size or not np.array_equal(have, want):
        raise ValueError("the last m columns of the graph are not the IRA staircase")
    u = np.asarray(info_bits)
    if u.shape[-1:] != (k,) or u.ndim not in (1, 2) or not np.isin(u, (0, 1)).all():
        raise ValueError(f"info_bits must be 0/1 of shape [{k}] or [B, {k}]")
    u2 = np.atleast_2d(u).astype(np.uint8)
    s = np.zeros((u2.shape[0], m), dtype=np.uint8)                                    # (H_info u)_i
    np.bitwise_xor.at(s, (slice(None), rows[~par]), u2[:, cols[~par]])
    c = np.concatenate([u2, np.bitwise_xor.accumulate(s, axis=1)], axis=1)
    return c[0] if u.ndim == 1 else c


def _is_staircase(graph: TannerGraph) -> bool:
    """the test of ``staircase_encode``: the last m columns are the IRA staircase and there is at least one information bit"""
    n, m = graph.n, graph.m
    k = n - m
    if k < 1 or m < 1:
        return False
    rows, cols = np.asarray(graph.check_of_edge, dtype=np.int64), np.asarray(graph.var_idx, dtype=np.int64)
    par = cols >= k
    have = np.unique(rows[par] * m + (cols[par] - k))
    p = np.arange(m, dtype=np.int64)
    want = np.unique(np.concatenate([p * m + p, (p[:-1] + 1) * m + p[:-1]]))
    return int(par.sum()) == want.size and np.array_equal(have, want)


class Encoder:
    """Systematic encoder of a binary linear code in the one format the device encoder reads (ldpc_encoder_create):

        p_r = XOR_{i in row r} u_i   (and, with ``accumulate`` and r > 0, XOR p_{r-1})
        c[info_pos[i]] = u_i,  c[parity_pos[r]] = p_r

    with ``row_ptr`` / ``info_idx`` a CSR over information-bit indices 0 .. k - 1, ``info_pos`` [k] and ``parity_pos``
    [n - k] ascending and together a permutation of 0 .. n - 1, and k = n - rank(H).  ``systematic``: the information bits
    are the first k code bits.  Build one with ``Encoder.from_graph``."""

    MAX_ENTRIES = 1 << 27

    def __init__(self, n: int, k: int, info_pos, parity_pos, row_ptr, info_idx, accumulate: bool):
        self.n, self.k = int(n), int(k)
        self.info_pos = np.ascontiguousarray(info_pos, dtype=np.int32)
        self.parity_pos = np.ascontiguousarray(parity_pos, dtype=np.int32)
        self.row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        self.info_idx = np.ascontiguousarray(info_idx, dtype=np.int32)
        self.accumulate = bool(accumulate)
        m = self.n - self.k
        if self.info_pos.shape != (self.k,) or self.parity_pos.shape != (m,) or self.row_ptr.shape != (m + 1,):
            raise ValueError("info_pos, parity_pos and row_ptr must have k, n - k and n - k + 1 entries")
        if not np.array_equal(np.sort(np.concatenate([self.info_pos, self.parity_pos])), np.arange(self.n)):
            raise ValueError("info_pos and parity_pos must together be a permutation of 0 .. n - 1")
        if (np.diff(self.info_pos) <= 0).any() or (np.diff(self.parity_pos) <= 0).any():
            raise ValueError("info_pos and parity_pos must be ascending")
        if self.row_ptr[0] != 0 or (np.diff(self.row_ptr) < 0).any() or int(self.row_ptr[-1]) != self.info_idx.size:
            raise ValueError("row_ptr must be monotone from 0 to len(info_idx)")
        if self.info_idx.size and (self.info_idx.min() < 0 or self.info_idx.max() >= self.k):
            raise ValueError("info_idx must hold information-bit indices 0 .. k - 1")
        self.systematic = bool(np.array_equal(self.info_pos, np.arange(self.k)))

    @classmethod
    def from_graph(cls, graph: TannerGraph, method: str = "auto") -> "Encoder":
        """method "auto": the sparse staircase form (rows = the information part of H, accumulate) when the last m columns
        are the IRA staircase -- the test of ``staircase_encode`` -- else "eliminate": Gauss-Jordan over GF(2) on the dense H,
        pivot columns searched from the highest column index down, for each column the first row at or below the current pivot
        row that has a 1; redundant rows drop out.  The pivot columns are the parity positions, the free columns the
        information positions, row r the free columns set in the reduced row of the r-th parity position.  ValueError when the
        CSR would exceed 2^27 entries (a large non-staircase code needs another encoder)."""
        if method not in ("auto", "eliminate"):
            raise ValueError(f"method must be 'auto' or 'eliminate', got {method!r}")
        n, m = graph.n, graph.m
        if method == "auto" and _is_staircase(graph):
            k = n - m
            rows, cols = np.asarray(graph.check_of_edge, dtype=np.int64), np.asarray(graph.var_idx, dtype=np.int64)
            info = cols < k
            order = np.lexsort((cols[info], rows[info]))
            row_ptr = np.zeros(m + 1, dtype=np.int64)
            np.cumsum(np.bincount(rows[info], minlength=m), out=row_ptr[1:])
            return cls(n, k, np.arange(k), np.arange(k, n), row_ptr, cols[info][order], True)
        A = graph.to_dense(np.uint8)
        r, pivots = 0, []
        for c in range(n - 1, -1, -1):
            if r == m:
                break
            hit = np.flatnonzero(A[r:, c])
            if hit.size == 0:
                continue
            p = r + int(hit[0])
            if p != r:
                A[[r, p]] = A[[p, r]]
            others = np.flatnonzero(A[:, c])
            others = others[others != r]
            A[others] ^= A[r]
            pivots.append(c)
            r += 1
        parity_pos = np.array(sorted(pivots), dtype=np.int64)
        is_par = np.zeros(n, dtype=bool)
        is_par[parity_pos] = True
        info_pos = np.flatnonzero(~is_par)
        k = n - r
        row_of_pivot = np.empty(n, dtype=np.int64)
        row_of_pivot[np.array(pivots, dtype=np.int64)] = np.arange(r)
        R = A[row_of_pivot[parity_pos]][:, info_pos] if r else np.zeros((0, k), dtype=np.uint8)
        entries = int(R.sum(dtype=np.int64))
        if entries > cls.MAX_ENTRIES:
            raise ValueError(f"the eliminated encoder has {entries} entries, more than 2^27: a large non-staircase code needs "
                             f"another encoder")
        row_ptr = np.zeros(r + 1, dtype=np.int64)
        np.cumsum(R.sum(axis=1, dtype=np.int64), out=row_ptr[1:])
        return cls(n, k, info_pos, parity_pos, row_ptr, np.nonzero(R)[1], False)

    def encode(self, info_bits) -> np.ndarray:
        """info_bits: 0/1, [k] or [B, k] -> uint8 codewords [n] or [B, n].  numpy, on the host: the yardstick of the device
        encoder; on a staircase graph it equals ``staircase_encode``."""
        u = np.asarray(info_bits)
        if u.shape[-1:] != (self.k,) or u.ndim not in (1, 2) or not np.isin(u, (0, 1)).all():
            raise ValueError(f"info_bits must be 0/1 of shape [{self.k}] or [B, {self.k}]")
        u2 = np.atleast_2d(u).astype(np.uint8)
        m = self.n - self.k
        p = np.zeros((u2.shape[0], m), dtype=np.uint8)
        row_of_entry = np.repeat(np.arange(m, dtype=np.int64), np.diff(self.row_ptr))
        np.bitwise_xor.at(p, (slice(None), row_of_entry), u2[:, self.info_idx])
        if self.accumulate:
            p = np.bitwise_xor.accumulate(p, axis=1)
        c = np.empty((u2.shape[0], self.n), dtype=np.uint8)
        c[:, self.info_pos] = u2
        c[:, self.parity_pos] = p
        return c[0] if u.ndim == 1 else c


if __name__ == "__main__":  # regenerate + verify the committed edge lists
    os.makedirs(_DATA_DIR, exist_ok=True)
    for name, spec in list(_SPECS.items()) + list(_QC_SPECS.items()):
        g = generate_qc_code(**spec) if name in _QC_SPECS else generate_ira_code(**spec)
        dvs = dict(zip(*np.unique(g.dv, return_counts=True)))
        dcs = dict(zip(*np.unique(g.dc, return_counts=True)))
        print(name, "n", g.n, "m", g.m, "E", g.E, "dv", dvs, "dc", dcs,
              "4-cycles", g.four_cycles() if g.E < 10000 else "n/a")
        p = _path(name)
        if name in _QC_SPECS:      # no file under data/: the recorded edge list is the test vector tests/golden/<name>.npz
            p = os.path.join(os.path.dirname(_DATA_DIR), os.pardir, "tests", "golden", name + ".npz")
            if not os.path.exists(p):
                print("   no recorded edge list to compare with")
                continue
        if os.path.exists(p):
            old = load_graph(p)
            same = np.array_equal(old.check_ptr, g.check_ptr) and np.array_equal(old.var_idx, g.var_idx) and \
                (old.layer_ptr is None) == (g.layer_ptr is None) and \
                (g.layer_ptr is None or np.array_equal(old.layer_ptr, g.layer_ptr))
            print("   committed file", "matches" if same else "DIFFERS (not overwritten)")
        else:
            save_graph(p, g)
            print("   wrote", p)
