"""
Codes, frame pools and batch arrangements shared by tests/test_tile_geometry_host.py (CPU: the graphs, the oracle and the
arrangements alone) and tests/test_gpu_tile_geometry.py (GPU): the streaming engine cuts a batch into tiles, and two launch
rules depend on how many there are -- which syndrome kernel runs with how many blocks per tile, and which tile mapping
cn_gather takes on what grid.  Nothing here says where those rules change: the GPU tests read that from
DecodeEngine.launch_geometry and assert that the tile counts below cross every change.  Not a test module: nothing here
needs a GPU.

Codes.  "m1100": a seeded graph of 1400 variables (degrees 1..8) and 1100 checks (degrees 3..8), small enough that the rows
one 256-codeword tile touches stay inside the budget of cn_gather's XCD mapping.  "m1100_hi": the same graph plus three
variables of degree 9, 12 and 20 on checks of the graph and one check of degree 40 on variables of the graph.  "small96": the
shipped 96 x 48 code.

Frames.  Every (code, precision) has one pool of POOL frames; a batch is an index vector into the pool (`arrangement`), so
every row of every batch has a known result: that of the same pool row decoded in a batch of a geometry the suite already
pins against the oracle.  The values are a seeded mix of the SNRs in MIX; by its class (CLASS, row i mod 8) a row is then
strongly sent (|llr| + 3: it stops at iteration 1), strongly sent but for three degree-1 variables with the wrong sign and a
larger magnitude than any message can reach (it never stops, and stays as tame numerically as a row that does: the
tolerance rule of the sum-product family shares one precision distance over the pool), rounded to quarters (ties between
magnitudes), given three exact zeros, or left as drawn.  tests/test_tile_geometry_host.py holds the conditions on what the
oracle makes of them.
"""
import functools
from collections import namedtuple

import numpy as np

import dirty_state_cases as ds
from dirty_state_cases import F32, F64, seed_of
from test_gpu_parity import oracle_capped

T = 6
POOL = 1024
N, M, EDGES = 1400, 1100, 5000
HI_VARS, HI_CHECK = (9, 12, 20), 40


# ---- codes ---------------------------------------------------------------------------------------------------------------
def _degrees(rng, count, lo, hi, total):
    """`count` degrees in lo..hi with the given sum, every value of lo..hi present"""
    d = np.concatenate([np.arange(lo, hi + 1), rng.integers(lo, hi + 1, count - (hi - lo + 1))])
    while d.sum() != total:
        step = 1 if d.sum() < total else -1
        ok = np.flatnonzero((d + step >= lo) & (d + step <= hi))
        ok = ok[ok >= hi - lo + 1]                               # the first hi - lo + 1 entries keep every degree present
        d[rng.choice(ok)] += step
    return d[rng.permutation(count)]


@functools.lru_cache(maxsize=None)
def m1100_edges():
    """-> (check of edge, variable of edge): every variable, highest degree first, goes to the dv checks with the most free
    sockets (ties at random), so both degree sequences are met exactly and no edge is doubled"""
    rng = np.random.default_rng(seed_of("m1100"))
    dv, free = _degrees(rng, N, 1, 8, EDGES), _degrees(rng, M, 3, 8, EDGES)
    rows, cols = [], []
    for j in np.argsort(-dv, kind="stable"):
        pick = np.lexsort((rng.random(M), -free))[:dv[j]]
        assert (free[pick] > 0).all()
        free[pick] -= 1
        rows += pick.tolist()
        cols += [int(j)] * int(dv[j])
    assert not free.any()
    return np.asarray(rows), np.asarray(cols)


def m1100():
    from ldpc_decoder import LDPCCode
    from tanner_graph import TannerGraph
    rows, cols = m1100_edges()
    return LDPCCode.from_graph(TannerGraph(N, M, rows, cols), k=N - M, max_iterations=T)


def m1100_hi():
    """m1100 plus variables N, N + 1, N + 2 of degree 9, 12 and 20, each on checks of degree <= 4 of its own, and check M of
    degree 40 on variables of degree 2..6 -- so the degrees of the old nodes stay within 3..8 and 1..8"""
    from ldpc_decoder import LDPCCode
    from tanner_graph import TannerGraph
    rows, cols = m1100_edges()
    rng = np.random.default_rng(seed_of("m1100_hi"))
    dc, dv = np.bincount(rows, minlength=M), np.bincount(cols, minlength=N)
    low = rng.permutation(np.flatnonzero(dc <= 4))[:sum(HI_VARS)]
    assert len(low) == sum(HI_VARS)
    new_rows, new_cols, at = [], [], 0
    for k, d in enumerate(HI_VARS):
        new_rows += low[at:at + d].tolist()
        new_cols += [N + k] * d
        at += d
    wide = rng.permutation(np.flatnonzero((dv >= 2) & (dv <= 6)))[:HI_CHECK]
    assert len(wide) == HI_CHECK
    new_rows += [M] * HI_CHECK
    new_cols += wide.tolist()
    g = TannerGraph(N + len(HI_VARS), M + 1, np.concatenate([rows, new_rows]), np.concatenate([cols, new_cols]))
    return LDPCCode.from_graph(g, k=g.n - g.m, max_iterations=T)


# the SNRs (dB) a pool mixes; chosen on the CPU from the oracle's counts alone (tests/test_tile_geometry_host.py holds the
# conditions)
MIX = {"tg-m1100": (3.0, 4.0, 5.5), "tg-m1100_hi": (3.0, 4.0, 5.5), "tg-small96": (1.0, 3.0, 5.0)}
ds.register_code("tg-m1100", m1100, T, (MIX["tg-m1100"][0], MIX["tg-m1100"][-1]))
ds.register_code("tg-m1100_hi", m1100_hi, T, (MIX["tg-m1100_hi"][0], MIX["tg-m1100_hi"][-1]))
ds.register_code("tg-small96", "small_96_48", T, (MIX["tg-small96"][0], MIX["tg-small96"][-1]))
CODES = ("tg-m1100", "tg-m1100_hi", "tg-small96")
GENERATED = ("tg-m1100", "tg-m1100_hi")
HI = "tg-m1100_hi"


# ---- families ------------------------------------------------------------------------------------------------------------
# name -> (family of tests/dirty_state_cases.py that builds the decoder and its seeded weights | "spa", engine mode,
#          precision, what DecodeEngine.info() reports as stream_form, codes)
# m1100_hi has variables of degree > 8: no fused RCQ iteration there (cn_gather takes dv <= 8)
Family = namedtuple("Family", "base mode dtype where codes")
FAMILIES = {
    "nms32": Family("basic32", "stream", F32, "two-sweeps", CODES),
    "n2d2": Family("n2d2", "stream", F32, "two-sweeps", CODES),                 # one beta per check degree and iteration, random
    "offset2": Family("offset2", "stream", F32, "two-sweeps", CODES),           # check-side alpha
    # the restatement of the sum-product pool on m1100_hi takes over a minute (a variable of degree 20): not run there
    "spa": Family("spa", "stream", F32, "two-sweeps", ("tg-m1100", "tg-small96")),
    "nms64": Family("basic64", "stream", F64, "two-sweeps", CODES),
    "wrcq-pair": Family("wrcq-q4", "pair", F32, "rcq-code-pair", CODES),
    "wrcq-gather": Family("wrcq-q4", "gather", F32, "fused-rcq-iteration", ("tg-m1100", "tg-small96")),
    "wrcq-sweeps": Family("wrcq-q4", "sweeps", F32, "two-sweeps", CODES),
}
FAMILY_CODES = [(f, c) for f, fam in FAMILIES.items() for c in fam.codes]
STOPS = (True, False)                                    # early stop | fixed T


def kind_of(family):
    base = FAMILIES[family].base
    return "spa" if base == "spa" else ds.FAMILIES[base].kind


def width(family):
    """codewords per tile of a batch above 64"""
    return 128 if FAMILIES[family].dtype is F64 else 256


_spa = {}


def decoder(family, code):
    base = FAMILIES[family].base
    if base != "spa":
        return ds.decoder(base, code)
    if code not in _spa:
        from ldpc_decoder import SumProductDecoder
        _spa[code] = SumProductDecoder(ds.load_code(code))
    return _spa[code]


def engine(family, code, device):
    """the family's engine on the code, forced to its streaming form"""
    fam = FAMILIES[family]
    if fam.base != "spa":
        return ds.engine(fam.base, code, device, fam.mode)
    return decoder(family, code)._get_engine(device).set_mode(fam.mode)


# ---- the pool --------------------------------------------------------------------------------------------------------------
STRONG, NEVER, ROUNDED, ZEROS, MIXED = range(5)
CLASS = np.asarray([STRONG, NEVER, NEVER, ROUNDED, ZEROS, MIXED, MIXED, MIXED])[np.arange(POOL) % 8]      # of pool row i
WRONG = 3                                                # wrongly sent degree-1 variables of a NEVER row (as many as there are)


def stuck_variables(graph):
    """degree-1 variables that are the only degree-1 variable of their check: sent strongly with the wrong sign, such a
    variable keeps its decision (its one message is weaker than its LLR) and no neighbour can flip with it into a codeword"""
    lone = graph.dv[graph.var_idx] == 1
    per_check = np.bincount(graph.check_of_edge[lone], minlength=graph.m)
    return np.sort(graph.var_idx[lone & (per_check[graph.check_of_edge] == 1)])


@functools.lru_cache(maxsize=None)
def pool(code, dtype=F32):
    """[POOL, n] read-only; the fp32 pool is the fp64 pool rounded"""
    graph = ds.load_code(code).tanner_graph()
    n = graph.n
    rng = np.random.default_rng(seed_of("pool", code))
    snr = np.asarray(MIX[code])[rng.integers(0, len(MIX[code]), POOL)]
    s2 = 10.0 ** (-snr / 10.0)[:, None]
    x = 2.0 * (1.0 + np.sqrt(s2) * rng.standard_normal((POOL, n))) / s2
    sure = (CLASS == STRONG) | (CLASS == NEVER)
    x[sure] = np.abs(x[sure]) + 3.0
    stuck = stuck_variables(graph)
    for i in np.flatnonzero(CLASS == NEVER):
        j = rng.choice(stuck, min(WRONG, len(stuck)), replace=False)
        x[i, j] = -(x[i, j] + 1000.0)
    r = CLASS == ROUNDED                                 # quarters, none of them zero
    x[r] = np.where(x[r] < 0, -1.0, 1.0) * np.maximum(np.round(4.0 * np.abs(x[r])) / 4.0, 0.25)
    for i in np.flatnonzero(CLASS == ZEROS):             # three exact zeros, on variables of degree >= 3
        x[i, rng.choice(np.flatnonzero(graph.dv >= 3), 3, replace=False)] = 0.0
    x = np.ascontiguousarray(x.astype(dtype))
    x.setflags(write=False)
    return x


def rows_of(cls):
    return np.flatnonzero(CLASS == cls)


# ---- what the pool decodes to ---------------------------------------------------------------------------------------------
Expected = namedtuple("Expected", "bits posterior iterations success keep bound")
_expected = {}


def expected(oracle_mod, family, code, early_stop):
    """the pool under the family's restatement: Expected(bits, posterior, iterations, success, keep, bound).  keep / bound are
    None except for the sum-product family: keep [POOL] the decisive frames (tests/spa_reference.py, non_decisive), bound
    [POOL, n] the 4 D_t bound of each frame's posterior against `posterior` (the float64 restatement's)."""
    key = (family, code, early_stop)
    if key in _expected:
        return _expected[key]
    kind, dec = kind_of(family), decoder(family, code)
    x = pool(code, FAMILIES[family].dtype)
    if kind == "spa":
        out = _spa_expected(code, early_stop)
    else:
        wkw = {}
        if kind != "basic":
            wkw = dict(wtype=ds.FAMILIES[FAMILIES[family].base].arg, beta={k: float(v.item()) for k, v in dec.beta_weights.items()},
                       alpha={k: float(v.item()) for k, v in dec.alpha_weights.items()})
        out = oracle_capped(oracle_mod, ds.oracle_graph(oracle_mod, ds.load_code(code)), x, kind, T, T, early_stop=early_stop, **wkw)
        out = Expected(*[np.asarray(a) for a in out[:4]], None, None)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    _expected[key] = out
    return out


@functools.lru_cache(maxsize=None)
def _spa_runs(code):
    """the float32 and the float64 restatement of the code's fp32 pool (tests/spa_reference.py), every iteration"""
    import spa_reference as R
    g = R.Graph.of(ds.load_code(code).tanner_graph())
    return R.decode(g, pool(code), T, np.float32), R.decode(g, pool(code), T, np.float64)


def _spa_expected(code, early_stop):
    import spa_reference as R
    lo, hi = _spa_runs(code)
    stop = hi["stop_iterations"] if early_stop else np.full(POOL, T, np.int32)
    flags, _ = R.non_decisive(lo, hi, stop)
    at = stop - 1
    post = hi["posterior"][at, np.arange(POOL)]
    bound = np.empty(post.shape, dtype=np.longdouble)
    for t in range(T):                                   # a frame whose outputs are those of iteration t: the bound of iteration t
        rows = at == t
        if rows.any():
            bound[rows] = R.tolerance(lo["posterior"][t], hi["posterior"][t], np.float32)[1][rows]
    bits = hi["bits"][at, np.arange(POOL)].astype(np.int32)
    success = hi["stop_success"] if early_stop else hi["ok"][T - 1]
    return Expected(bits, post, stop.astype(np.int32), success.copy(), ~flags, bound)


# ---- arrangements ----------------------------------------------------------------------------------------------------------
TILES = (5, 15, 16, 17, 23, 24, 51, 52, 63, 64, 65)
RUN_ORDER = (65, 5, 64, 17, 63, 16, 52, 15, 51, 24, 23)    # every decode inherits the scratch of another tile count
assert sorted(RUN_ORDER) == list(TILES)
# what a family may cut its list to: the neighbours of every tile count at which a launch rule can change
NEIGHBOURS = (15, 16, 17, 51, 52, 63, 64, 65)

Arrangement = namedtuple("Arrangement", "tiles W B index strong_tile never_tile mixed_tile")


def ragged(tiles, W):
    """how many frames the last tile lacks: 0, 1, W - 1 in rotation over TILES"""
    return (0, 1, W - 1)[TILES.index(tiles) % 3]


@functools.lru_cache(maxsize=None)
def arrangement(tiles, W):
    """B = tiles * W - ragged frames as indices into the pool.  Three full tiles at seeded places hold strongly sent frames
    only, frames that never stop only, and one frame of every class in turn; every other place draws from the whole pool (in
    the largest arrangement every pool row first).  Where the last tile holds a single frame it is a strongly sent one."""
    rng = np.random.default_rng(seed_of("arrangement", tiles, W))
    B = tiles * W - ragged(tiles, W)
    strong_tile, never_tile, mixed_tile = (int(t) for t in rng.permutation(tiles - 1)[:3])
    index = rng.integers(0, POOL, tiles * W)
    special = np.zeros(tiles * W, dtype=bool)
    for tile, rows in ((strong_tile, rows_of(STRONG)), (never_tile, rows_of(NEVER)), (mixed_tile, np.arange(POOL))):
        index[tile * W:(tile + 1) * W] = rows[(np.arange(W) + rng.integers(0, len(rows))) % len(rows)]
        special[tile * W:(tile + 1) * W] = True
    special[B - 1:] = True
    free = np.flatnonzero(~special)
    if len(free) >= POOL:
        index[rng.permutation(free)[:POOL]] = rng.permutation(POOL)
    if B % W == 1:
        index[B - 1] = rng.choice(rows_of(STRONG))
    index = np.ascontiguousarray(index[:B])
    index.setflags(write=False)
    return Arrangement(tiles, W, B, index, strong_tile, never_tile, mixed_tile)


def arrangements(family, order=RUN_ORDER):
    return [arrangement(t, width(family)) for t in order]
