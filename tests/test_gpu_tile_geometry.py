"""
A streaming decode does not depend on how many tiles its batch is cut into.  Two launch rules do (csrc/ldpc_hip.hip,
syndrome_chunks and gather_tiles): below some tile count the syndrome + latch pass runs several blocks per tile, which meet
through a per-tile ticket and an OR word in the workspace, and from some tile count on cn_gather deals its tiles to the XCDs on
a grid padded to a multiple of 8.  tests/tile_geometry_cases.py has the codes, the pool of frames and the batch arrangements
(index vectors into the pool, 5 to 65 tiles, ragged last tiles, a tile that is done at once beside one that never is);
tests/test_tile_geometry_host.py what the restatements make of them.

(a) pins the pool to the restatement of its family at B = 1000 and B = 24, geometries the suite already runs, under the
suite's standing comparison (the only host-side one here).  (b) decodes every arrangement, twice in a row, on one engine and
one workspace, and compares on the device with the pool's outputs gathered by the same index: a codeword's arithmetic does
not depend on the geometry, so equality is bit for bit.  (c) asserts through DecodeEngine.launch_geometry that the tile
counts cross every change of the two rules -- nothing in the tests restates where they lie.  (d): every row reported as a
success satisfies every check, on the code with variables of degree above 8.  (e): the C entry point with exactly the
workspace it asks for, inside a larger buffer that must stay untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import tile_geometry_cases as tg
from tile_geometry_cases import ds
from test_gpu_parity import assert_post

pytestmark = pytest.mark.gpu

FIELDS = ("bits", "posterior", "iterations", "success", "packed_bits")
IDS = [f"{f}-{c}" for f, c in tg.FAMILY_CODES]


@pytest.fixture(autouse=True)
def inference_mode():
    with torch.no_grad():
        yield


def engine(family, code, dev):
    """the family's engine, forced to its streaming form, with what info() must then report"""
    eng = tg.engine(family, code, dev)
    info = eng.info()
    assert info["engine"] == "stream" and info["stream_form"] == tg.FAMILIES[family].where, info
    assert info["form"] == {"basic": "NMS", "neural2d": "NMS", "offset": "OMS", "spa": "SPA", "wrcq": "RCQ"}[tg.kind_of(family)], info
    return eng


_device = {}


def on_device(key, make):
    if key not in _device:
        _device[key] = make()
    return _device[key]


def pool_on(family, code, dev):
    dt = tg.FAMILIES[family].dtype
    return on_device(("pool", code, dt), lambda: torch.from_numpy(np.array(tg.pool(code, dt))).to(dev))


def fields(res):
    return {k: getattr(res, k) for k in FIELDS}


def pool_outputs(family, code, early_stop, dev):
    """the five outputs of the whole pool on the device: rows 0..999 decoded as one batch of 1000, rows 1000..1023 as one of
    24 -- the two geometries test (a) compares with the restatement"""
    def make():
        eng, x = engine(family, code, dev), pool_on(family, code, dev)
        parts = [fields(eng.decode(x[lo:hi].clone(), early_stop=early_stop, want_packed=True)) for lo, hi in ((0, 1000), (1000, tg.POOL))]
        return {k: torch.cat([p[k] for p in parts]) for k in FIELDS}
    return on_device(("out", family, code, early_stop), make)


def raw(t):
    """a tensor's bits: equality below is bit for bit (-0.0 is not 0.0)"""
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64) if t.is_floating_point() else t


def same_on_device(got, want, tag):
    for k in FIELDS:
        assert got[k].shape == want[k].shape and torch.equal(raw(got[k]), raw(want[k])), f"{tag}: {k} differs from the pool's"


# ---- a. the pool against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,code", tg.FAMILY_CODES, ids=IDS)
def test_a_the_pool_decodes_as_the_restatement_says(family, code, gpu_device, oracle_mod):
    kind, n = tg.kind_of(family), ds.load_code(code).n
    for early_stop in tg.STOPS:
        want = tg.expected(oracle_mod, family, code, early_stop)
        got = {k: v.cpu().numpy() for k, v in pool_outputs(family, code, early_stop, gpu_device).items()}
        tag = f"{family} on {code}, early_stop={early_stop}"
        rows = np.ones(tg.POOL, bool) if want.keep is None else want.keep
        np.testing.assert_array_equal(got["iterations"][rows], want.iterations[rows], err_msg=tag)
        np.testing.assert_array_equal(got["success"][rows], want.success[rows], err_msg=tag)
        np.testing.assert_array_equal(got["bits"][rows], want.bits[rows], err_msg=tag)
        expanded = np.unpackbits(got["packed_bits"], axis=1, bitorder="little")
        assert not expanded[:, n:].any(), f"{tag}: the pad bits of a packed row are zero"
        np.testing.assert_array_equal(expanded[:, :n], got["bits"], err_msg=f"{tag}: packed bits")
        if kind == "spa":
            err = np.abs(got["posterior"].astype(np.longdouble) - want.posterior.astype(np.longdouble))
            print(f"{tag}: largest posterior error {float(err[rows].max()):.3g} on {int(rows.sum())} decisive frames")
            assert (err[rows] <= want.bound[rows]).all(), (tag, float(err[rows].max()))
        elif kind in ds.EXACT_POSTERIOR or tg.FAMILIES[family].dtype is tg.F64:
            np.testing.assert_array_equal(got["posterior"], want.posterior, err_msg=tag)
        else:
            assert_post(got["posterior"], want.posterior, tag)
        assert len(np.unique(got["iterations"])) >= (3 if early_stop else 1)


# ---- b. every arrangement, on the device ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,code", tg.FAMILY_CODES, ids=IDS)
def test_b_every_arrangement_decodes_as_the_pool_does(family, code, gpu_device):
    eng, x = engine(family, code, gpu_device), pool_on(family, code, gpu_device)
    runs = tg.arrangements(family)
    assert runs[0].tiles == max(tg.TILES)                        # the first decode sizes the workspace every later one reuses
    for early_stop in tg.STOPS:
        pool = pool_outputs(family, code, early_stop, gpu_device)
        ws = None
        for a in runs:
            assert eng.launch_geometry(a.B)["tiles"] == a.tiles
            index = torch.from_numpy(np.array(a.index)).to(gpu_device)
            llr = x[index]
            want = {k: v[index] for k, v in pool.items()}
            for again in (False, True):
                got = fields(eng.decode(llr, early_stop=early_stop, want_packed=True))
                same_on_device(got, want, f"{family} on {code}, early_stop={early_stop}, {a.tiles} tiles, B={a.B}, again={again}")
            here = eng._workspace(a.B).data_ptr()
            assert ws in (None, here)                            # one workspace: each decode inherits another tile count's scratch
            ws = here
            if early_stop:                                       # the special tiles did what they are there for
                tile = lambda t: got["iterations"][t * a.W:(t + 1) * a.W]
                assert bool((tile(a.strong_tile) == 1).all()) and bool((tile(a.never_tile) == tg.T).all())
                assert len(torch.unique(tile(a.mixed_tile))) >= 3


# ---- c. the tile counts cross every change of the two launch rules -----------------------------------------------------------------
@pytest.mark.parametrize("family,code", tg.FAMILY_CODES, ids=IDS)
def test_c_the_arrangements_cross_every_threshold(family, code, gpu_device):
    eng = engine(family, code, gpu_device)
    W = tg.width(family)
    geo = {}
    for a in tg.arrangements(family, tg.TILES):
        geo[a.tiles] = g = eng.launch_geometry(a.B)
        assert (g["vec"], g["tiles"]) == (W // 64, a.tiles), g
        assert eng.launch_geometry(a.tiles * W) == g             # the ragged last tile changes nothing
    chunks = {t: g["syndrome_chunks"] for t, g in geo.items()}
    if code in tg.GENERATED:
        # five blocks of 256 checks: all five while the grid stays small, four from 52 tiles, the one-block kernel from 64
        assert set(chunks.values()) == {5, 4, 1}, chunks
        assert [chunks[t] for t in (5, 15, 16, 17, 23, 24, 51)] == [5] * 7 and (chunks[52], chunks[63]) == (4, 4), chunks
        assert (chunks[64], chunks[65]) == (1, 1), chunks
    else:
        assert set(chunks.values()) == {1}, chunks               # m = 48: one block of checks, the one-block kernel throughout
    xcd = {t: g["gather_xcd_tiles"] for t, g in geo.items()}
    padded = {t: g["gather_tiles_padded"] for t, g in geo.items()}
    if tg.FAMILIES[family].mode == "gather":
        assert xcd[5] == 0 and xcd[15] == 0 and all(xcd[t] == t for t in tg.TILES if t >= 16), xcd
        assert all(padded[t] == t for t in (5, 15, 16, 24, 64)), padded
        assert padded[17] > 17 and padded[23] > 23 and all(padded[t] % 8 == 0 and t <= padded[t] < t + 8 for t in tg.TILES if t >= 16), padded
    else:
        assert not any(xcd.values()) and all(padded[t] == t for t in tg.TILES), (xcd, padded)


def test_c_launch_geometry_refusals(gpu_device):
    eng = engine("nms32", "tg-small96", gpu_device)
    assert eng._lib.ldpc_debug_launch_geometry(eng.handle, 65, None) == -1                   # NULL output: LDPC_ERR_ARG
    with pytest.raises(ValueError):
        eng.launch_geometry(0)
    assert eng.launch_geometry(64) == {"vec": 1, "tiles": 1, "syndrome_chunks": 1, "gather_xcd_tiles": 0, "gather_tiles_padded": 1}
    try:
        eng.set_mode("auto")
        assert eng.info()["engine"] == "resident"
        with pytest.raises(NotImplementedError):                 # LDPC_ERR_UNSUPPORTED: no tiles on an LDS-resident engine
            eng.launch_geometry(65)
    finally:
        eng.set_mode("stream")


# ---- d. success = 1 => H bits = 0, variables of degree above 8 included -----------------------------------------------------------
@pytest.mark.parametrize("family", [f for f, c in tg.FAMILY_CODES if c == tg.HI])
def test_d_every_row_reported_as_a_success_satisfies_every_check(family, gpu_device):
    """vn_last_rows rewrites the rows of codewords the latch froze earlier; on m1100_hi the variables of degree 9, 12 and 20
    take its generic_post path.  The syndrome is computed on the device from the graph."""
    code = tg.HI
    eng, x = engine(family, code, gpu_device), pool_on(family, code, gpu_device)
    graph = ds.load_code(code).tanner_graph()
    assert graph.dv.max() == 20
    Ht = torch.from_numpy(graph.to_dense(np.float32).T.copy()).to(gpu_device)          # sums of at most 40 ones: exact in fp32
    a = tg.arrangement(17, tg.width(family))
    llr = x[torch.from_numpy(np.array(a.index)).to(gpu_device)]
    wide = torch.from_numpy(np.flatnonzero(graph.dv > 8)).to(gpu_device)
    for early_stop in tg.STOPS:
        for cap in (None, 3):
            res = eng.decode(llr, early_stop=early_stop, want_packed=True, max_iters=cap)
            tag = f"{family}, early_stop={early_stop}, max_iters={cap}"
            unsat = (res.bits.to(torch.float32) @ Ht).remainder(2).any(dim=1)
            ok = res.success
            assert bool(ok.any()) and not bool(ok.all()), tag
            assert not bool((ok & unsat).any()), f"{tag}: a row reported as a success fails a check"
            assert torch.equal(ok, ~unsat), f"{tag}: success is the syndrome of the returned decisions"
            assert bool((res.iterations[~ok] == (cap or tg.T)).all()), tag
            if early_stop:
                assert len(torch.unique(res.iterations[ok])) >= 2, tag          # rows the latch froze earlier than others
            unpacked = (res.packed_bits[:, (wide // 8)] >> (wide % 8).to(torch.uint8)) & 1
            assert torch.equal(unpacked.to(torch.int32), res.bits[:, wide]), tag
            assert torch.equal(res.bits, (res.posterior < 0).to(torch.int32)), tag


# ---- e. exactly the workspace the library asks for ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family,code", [(f, c) for f, c in tg.FAMILY_CODES if c == ("tg-m1100" if "tg-m1100" in tg.FAMILIES[f].codes else tg.HI)],
                         ids=lambda v: v)
def test_e_a_decode_stays_inside_the_workspace_it_asked_for(family, code, gpu_device):
    import _native as nat
    eng, x = engine(family, code, gpu_device), pool_on(family, code, gpu_device)
    early_stop = True
    pool = pool_outputs(family, code, early_stop, gpu_device)
    a = tg.arrangement(17, tg.width(family))
    index = torch.from_numpy(np.array(a.index)).to(gpu_device)
    llr, want = x[index].contiguous(), {k: v[index] for k, v in pool.items()}
    B, n = llr.shape
    need = eng.workspace_bytes(B)
    big = torch.full((3 * need + 512,), 0xA5, dtype=torch.uint8, device=gpu_device)
    lo = (big.data_ptr() + need + 255) // 256 * 256 - big.data_ptr()          # a 256-byte boundary, a workspace's worth of filler before it
    hi = lo + need
    assert lo >= need and big.numel() - hi >= need and (big.data_ptr() + lo) % 256 == 0

    def outputs(fill):
        return {"bits": torch.full((B, n), fill, dtype=torch.int32, device=gpu_device),
                "posterior": torch.full((B, n), float(fill), dtype=eng.dtype, device=gpu_device),
                "iterations": torch.full((B,), fill, dtype=torch.int32, device=gpu_device),
                "success": torch.full((B,), fill, dtype=torch.uint8, device=gpu_device),
                "packed_bits": torch.full((B, (n + 7) // 8), fill, dtype=torch.uint8, device=gpu_device)}

    def call(out, nbytes):
        p = lambda t: C.c_void_p(t.data_ptr())
        with torch.cuda.device(gpu_device):
            stream = torch.cuda.current_stream(gpu_device).cuda_stream
            return eng._lib.ldpc_decode(eng.handle, p(llr), B, int(early_stop), *[p(out[k]) for k in FIELDS],
                                        C.c_void_p(big.data_ptr() + lo), nbytes, C.c_void_p(stream))

    out = outputs(77)
    nat.check(call(out, need), "ldpc_decode")
    assert bool((big[:lo] == 0xA5).all()) and bool((big[hi:] == 0xA5).all()), "bytes outside the workspace were written"
    assert not bool((big[lo:hi] == 0xA5).all())
    out["success"] = out["success"].bool()
    same_on_device(out, want, f"{family} on {code}: a workspace of exactly {need} bytes")
    # one byte less: refused before anything is launched
    big.fill_(0xA5)
    out = outputs(77)
    assert call(out, need - 1) == -4                             # LDPC_ERR_WORKSPACE
    torch.cuda.synchronize(gpu_device)
    assert bool((big == 0xA5).all())
    assert all(bool((raw(out[k]) == raw(torch.full_like(out[k], 77))).all()) for k in FIELDS)
