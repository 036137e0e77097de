"""
GPU tests (-m gpu) of pass 1 of the resident check phase taken two edges at a time (csrc/ldpc_resident.hip, res_absorb2:
min3 / med3 / min on the magnitudes and a three-input xor on the signs, an odd last edge through the one-value step).

Hook test: ldpc_debug_min2 runs the one-value chain and the pair form on rows of d = 1 .. 32 values; both must give numpy's
two smallest magnitudes and the xor of the bit patterns, bit for bit, on a pool of special values and on 200,000 rows of
random bit patterns (NaN patterns replaced by +-inf: NaN is outside the decoders' domain).

Decode test: Basic, Neural-2D (sharing type 2) and RCQ (bc = 3) on the codes `tails` and `fallback` of
test_gpu_compact_checks, `spread` of test_gpu_compact_grid and small_96_48 -- odd and even check degrees, degree-1 and
degree-2 checks, mixed-degree and partly filled waves, scalar-counted next to per-lane waves -- at B = 37 and B = 1.  The
check inputs of iteration 1 are the LLRs themselves, so the rows of the batch are built as check inputs: integers (ties in
every later iteration too), one magnitude everywhere, the minimum of a check at its first, its last and its odd-tail edge
in the KERNEL's edge order (the rows of the plan's slot placement), zeros of both signs, +-inf and subnormals.  Every
row is compared: per-edge C2V after 1 and 3 iterations with the streaming engine (bitwise; as codes for RCQ), the T = 10
decode with the streaming engine and the CPU oracle, and once more with early_stop=True (the general kernel).
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _native
from test_gpu_compact_checks import make_code as checks_code
from test_gpu_compact_forms import assert_c2v_equal
from test_gpu_compact_grid import POST_TOL, make_code as grid_code
from test_gpu_parity import QP, oracle_capped

pytestmark = pytest.mark.gpu

assert POST_TOL == 1e-5
f32 = np.float32


@pytest.fixture(autouse=True)
def inference_mode(monkeypatch):
    monkeypatch.setenv("LDPC_ENGINE_MODE", "auto")
    with torch.no_grad():
        yield


# ---- the hook: both device forms against numpy ------------------------------------------------------------------------------
SPECIAL = np.asarray([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 3e-39, -3e-39, 1.1754944e-38, -1.1754944e-38, 3.4e38,
                      -3.4e38, 1.0, -1.0, 2.5, 0.7], f32)
RANDOM_ROWS = 200_000
_pool = {}


def random_rows():
    """[RANDOM_ROWS, 32] random bit patterns, a NaN pattern replaced by the infinity of its sign; made once"""
    if "rnd" not in _pool:
        rng = np.random.default_rng(1401)
        bits = rng.integers(0, 2 ** 32, (RANDOM_ROWS, 32), dtype=np.uint64).astype(np.uint32)
        nan = (bits & 0x7fffffff) > 0x7f800000
        bits[nan] = (bits[nan] & np.uint32(0x80000000)) | np.uint32(0x7f800000)
        _pool["rnd"] = bits.view(f32)
        assert not np.isnan(_pool["rnd"]).any()
    return _pool["rnd"]


def special_rows(d):
    """all-equal rows of every special value, rows drawn from the special values alone (ties of the two and of the three
    smallest, zeros of both signs, infinities, subnormals), and rows of distinct magnitudes whose smallest is written to two
    and to three places (d permitting)"""
    rng = np.random.default_rng(1500 + d)
    rows = [np.repeat(SPECIAL[:, None], d, axis=1), SPECIAL[rng.integers(0, len(SPECIAL), (4096, d))]]
    for copies in (2, 3):
        if d >= copies:
            x = (rng.uniform(1.0, 9.0, (512, d)) * rng.choice([-1.0, 1.0], (512, d))).astype(f32)
            lo = np.abs(x).min(axis=1)
            for r in range(len(x)):
                at = rng.choice(d, copies, replace=False)
                x[r, at] = lo[r] * rng.choice([-1.0, 1.0], copies)
            rows.append(x)
    return np.concatenate(rows).astype(f32)


def run_min2(vals, gpu_device):
    lib = _native.load()
    rows, d = vals.shape
    x = torch.from_numpy(np.ascontiguousarray(vals)).to(gpu_device)
    out = []
    for _ in range(2):
        out.append(torch.full((rows, 2), -1.0, dtype=torch.float32, device=gpu_device))
        out.append(torch.full((rows,), 0x5a5a5a5a, dtype=torch.int32, device=gpu_device))
    rc = lib.ldpc_debug_min2(C.c_void_p(x.data_ptr()), rows, d, *[C.c_void_p(o.data_ptr()) for o in out],
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    m12c, parc, m12p, parp = [o.cpu().numpy() for o in out]
    return (m12c, parc.view(np.uint32)), (m12p, parp.view(np.uint32))


@pytest.mark.parametrize("d", list(range(1, 33)))
def test_min2_hook_both_forms_equal_numpy(d, gpu_device):
    vals = np.concatenate([special_rows(d), np.ascontiguousarray(random_rows()[:, :d])])
    assert len(vals) >= RANDOM_ROWS and not np.isnan(vals).any()
    mag = np.sort(np.abs(vals), axis=1)
    want = np.full((len(vals), 2), np.inf, f32)
    want[:, 0] = mag[:, 0]
    if d > 1:
        want[:, 1] = mag[:, 1]                       # d == 1: m2 stays +inf, the hook applies no degree-1 rule
    par = np.bitwise_xor.reduce(vals.view(np.uint32), axis=1)
    sign = np.bitwise_xor.reduce(np.signbit(vals), axis=1)
    assert np.array_equal(par >> 31, sign.astype(np.uint32))
    for form, (m12, got_par) in zip(("chain", "pairs"), run_min2(vals, gpu_device)):
        bad = (m12.view(np.uint32) != want.view(np.uint32)).any(axis=1)
        assert not bad.any(), f"{form}, d = {d}: (m1, m2) of {int(bad.sum())} rows differ, first row {vals[bad][0]}"
        assert np.array_equal(got_par, par), f"{form}, d = {d}: parity word"


def test_min2_hook_refuses_bad_arguments(gpu_device):
    lib = _native.load()
    x = torch.zeros(8, dtype=torch.float32, device=gpu_device)
    p = C.c_void_p(x.data_ptr())
    assert lib.ldpc_debug_min2(p, 1, 0, p, p, p, p, None) == -1
    assert lib.ldpc_debug_min2(p, 1, 33, p, p, p, p, None) == -1
    assert lib.ldpc_debug_min2(p, 0, 4, p, p, p, p, None) == -1
    assert lib.ldpc_debug_min2(None, 1, 4, p, p, p, p, None) == -1


# ---- decodes whose check inputs are built --------------------------------------------------------------------------------
CODES = ["tails", "fallback", "spread", "small_96_48"]
DECODERS = ["basic", "neural2d", "rcq"]
B_FULL, T_FULL = 37, 10
KINDS = ["integers", "one-magnitude", "min-first", "min-last", "min-tail", "min-rotating", "zeros", "inf", "subnormal",
         "integers-wide"]
_cache = {}


def make_code(name, T=T_FULL):
    if name == "small_96_48":
        import codes
        return codes.load_code("small_96_48", max_iterations=T)
    return checks_code(name, T) if name in ("tails", "fallback") else grid_code(name, T)


def build(name, decoder, gpu_device):
    """-> (code, decoder object, engine, oracle keyword arguments), one per (code, decoder) and process"""
    key = (name, decoder)
    if key not in _cache:
        from ldpc_decoder import BasicMinSumDecoder
        from neural_2d_decoder import Neural2DMinSumDecoder
        from rcq_decoder import RCQMinSumDecoder
        code = make_code(name)
        if decoder == "basic":
            dec = BasicMinSumDecoder(code, 0.7)
            eng, okw = dec._engine(torch.float32, gpu_device), dict(factor=0.7)
        elif decoder == "neural2d":
            rng = np.random.default_rng(1402)
            dec = Neural2DMinSumDecoder(code, weight_sharing_type=2, max_iterations=T_FULL)
            for p in dec.beta_weights.values():
                p.fill_(float(f32(rng.uniform(0.5, 1.0))))
            for p in dec.alpha_weights.values():
                p.fill_(float(f32(rng.uniform(0.8, 1.2))))
            eng = dec._get_engine(gpu_device)
            okw = dict(wtype=2, beta={k: float(v.item()) for k, v in dec.beta_weights.items()},
                       alpha={k: float(v.item()) for k, v in dec.alpha_weights.items()})
        else:
            dec = RCQMinSumDecoder(code, 3, 8, QP, T_FULL)
            eng, okw = dec._get_engine(gpu_device), dict(bc=3, qp=QP)
        eng.set_mode("auto")
        _cache[key] = (code, dec, eng, okw)
    return _cache[key]


def kernel_rows(eng, code):
    """row (position in the kernel's edge order) of every edge in CSR order, from the slot placement the plan ships"""
    g = code.tanner_graph()
    slot = np.full(g.E, -1, np.int32)
    geom = np.zeros(2, np.int32)
    rc = eng._lib.ldpc_debug_compact_banks(eng.handle, 0, 0, 0, None, None, _native.ptr(slot), None, None, None, None, None,
                                           _native.ptr(geom))
    assert rc == 0, "the engine has no compact plan"
    row = slot // int(geom[0])
    dc = np.diff(g.check_ptr)
    for c in range(len(dc)):                                     # a check's edges fill rows 0 .. dc-1
        assert sorted(row[g.check_ptr[c]: g.check_ptr[c + 1]]) == list(range(dc[c]))
    return row


def place_minima(rng, g, row, x, where):
    """lower one variable per check to a magnitude below every other one so that the check's minimum sits at kernel row
    `where(dc, index of the check)`; a check is taken when none of its variables was lowered for another check"""
    dc = np.diff(g.check_ptr)
    lowered = np.zeros(g.n, bool)
    taken = 0
    for c in rng.permutation(len(dc)):
        e = np.arange(g.check_ptr[c], g.check_ptr[c + 1])
        if lowered[g.var_idx[e]].any():
            continue
        v = g.var_idx[e[row[e] == where(int(dc[c]), int(c))][0]]
        x[v] = np.sign(x[v]) * f32(0.01 + 0.9 * rng.random())    # the others are >= 1
        lowered[v] = True
        taken += 1
    assert taken >= min(8, len(dc) // 8)
    return x


def inf_variables(rng, g, count):
    """variables that may hold an infinite LLR: every one of their checks has degree >= 3 and no other such variable, so
    every message into them stays finite and no inf - inf arises"""
    dc = np.diff(g.check_ptr)
    chk_of_edge = np.repeat(np.arange(len(dc)), dc)
    used = np.zeros(len(dc), bool)
    out = []
    for v in rng.permutation(g.n):
        cs = chk_of_edge[g.var_idx == v]
        if len(cs) and (dc[cs] >= 3).all() and not used[cs].any():
            used[cs] = True
            out.append(v)
            if len(out) == count:
                break
    assert out
    return np.asarray(out)


def inputs(name, eng, code):
    """[B_FULL, n] LLRs, row r of kind KINDS[r % len(KINDS)]"""
    if ("llr", name) in _cache:
        return _cache[("llr", name)]
    g = code.tanner_graph()
    row = kernel_rows(eng, code)
    n = g.n
    out = np.zeros((B_FULL, n), f32)
    for r in range(B_FULL):
        rng = np.random.default_rng(1410 + r)
        kind = KINDS[r % len(KINDS)]
        flip = (0.12, 0.04, 0.01)[r % 3]                       # sent word: all zero; the cleaner rows decode
        sign = rng.choice([-1.0, 1.0], n, p=[flip, 1.0 - flip]).astype(f32)
        normal = (sign * rng.uniform(1.0, 9.0, n)).astype(f32)
        if kind == "integers":
            x = np.round(rng.standard_normal(n) * 2.0 + 2.0).astype(f32)          # exact zeros among them
        elif kind == "integers-wide":
            x = (sign * rng.integers(1, 4, n)).astype(f32)
        elif kind == "one-magnitude":
            x = sign * f32(2.5)
        elif kind == "min-first":
            x = place_minima(rng, g, row, normal, lambda dc, c: 0)
        elif kind == "min-last":
            x = place_minima(rng, g, row, normal, lambda dc, c: dc - 1)
        elif kind == "min-tail":                                                  # the last even row: the odd tail of an odd
            x = place_minima(rng, g, row, normal, lambda dc, c: 2 * ((dc - 1) // 2))   # degree (and of d_lo = dc - 1)
        elif kind == "min-rotating":
            x = place_minima(rng, g, row, normal, lambda dc, c: c % dc)
        elif kind == "zeros":
            x = normal.copy()
            z = rng.random(n) < 0.15
            x[z] = np.where(rng.random(int(z.sum())) < 0.5, f32(-0.0), f32(0.0))
        elif kind == "inf":
            x = normal.copy()
            at = inf_variables(rng, g, 12)
            x[at] = np.where(x[at] < 0, -np.inf, np.inf)
        else:
            x = normal.copy()
            s = rng.random(n) < 0.3
            x[s] = (np.sign(x[s]) * rng.choice([1e-45, 3e-39, 1.1754942e-38, 7e-42], int(s.sum()))).astype(f32)
        out[r] = x
    assert set(KINDS) == {KINDS[r % len(KINDS)] for r in range(B_FULL)}
    _cache[("llr", name)] = out
    return out


def assert_compact_ran(eng):
    info = eng.info()
    assert info["engine"] == "resident" and info["compact_plan"] is not None
    k = info["resident_kernel"]["fixed_T"]
    assert k["plan"] == "compact" and k["G"] == 2 and not k["split"] and k["ms"] == k["row_stride"] == 495
    assert info["resident_kernel"]["early_stop"]["plan"] != "compact"
    return k


def assert_post(got, want, exact):
    """POST_TOL relative to max(1, |ref|) where the reference is finite, the same infinity where it is not"""
    got, want = np.asarray(got), np.asarray(want)
    assert not np.isnan(want).any(), "the inputs were built so that no inf - inf arises"
    if exact:
        np.testing.assert_array_equal(got, want)
        return
    fin = np.isfinite(want)
    np.testing.assert_array_equal(got[~fin], want[~fin])
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    assert np.all(err <= POST_TOL * np.maximum(1.0, np.abs(want[fin]))), f"posterior max err {err.max()}"


def assert_equals_oracle(res, want, exact):
    ob, op, oi, os_ = want[:4]
    np.testing.assert_array_equal(res.bits.cpu().numpy(), ob)
    np.testing.assert_array_equal(res.iterations.cpu().numpy(), oi)
    np.testing.assert_array_equal(res.success.cpu().numpy().astype(bool), os_)
    assert_post(res.posterior.cpu().numpy(), op, exact)


def both_engines(eng, x, early_stop):
    eng.set_mode("auto")
    a = eng.decode(x, early_stop=early_stop, want_packed=True)
    eng.set_mode("stream")
    b = eng.decode(x, early_stop=early_stop, want_packed=True)
    eng.set_mode("auto")
    for f in ("bits", "posterior", "iterations", "success", "packed_bits"):      # as test_gpu_compact_grid.assert_same_as_stream
        assert torch.equal(getattr(a, f), getattr(b, f)), f
    return a


@pytest.mark.parametrize("B", [B_FULL, 1])
@pytest.mark.parametrize("decoder", DECODERS)
@pytest.mark.parametrize("name", CODES)
def test_decode_of_built_check_inputs(name, decoder, B, gpu_device, oracle_mod):
    code, dec, eng, okw = build(name, decoder, gpu_device)
    k = assert_compact_ran(eng)
    assert k["form"] == ("RCQ" if decoder == "rcq" else "NMS") and k["bpc"]
    llr = inputs(name, eng, code)
    if B == 1:
        llr = llr[KINDS.index("min-tail")][None].copy()
    x = torch.from_numpy(llr).to(gpu_device)
    g = code.tanner_graph()
    og = oracle_mod.OracleGraph(n=g.n, check_ptr=g.check_ptr, var_idx=g.var_idx)
    for cap in (1, 3):
        assert_c2v_equal(dec, eng, x, cap)
    for early_stop in (False, True):
        res = both_engines(eng, x, early_stop)
        want = oracle_capped(oracle_mod, og, llr, decoder, T_FULL, T_FULL, early_stop=early_stop, **okw)
        assert_equals_oracle(res, want, decoder == "rcq")
