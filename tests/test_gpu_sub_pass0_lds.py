"""Phase A of the column form of iteration 0 (tile_sub.hip sub_pass0_cols)
gathers the A columns' tanh table from LDS: sub_tanh_table stages it in the S
region, the row products wait in their rows' identity-edge slots of E until the
table is dead, and a sub-tile that loses the tiny-|t| vote re-zeroes S before
its row pipeline.  LDPC_PASS0_LDS=0 keeps the gather from global memory.

Nothing changes a bit: every output -- hard bits, convergence iteration,
Result, iterations, normalized LLR and its history, posteriors, messages -- must
be IDENTICAL with the switch on and off and to the split path's
(decode(..., split=True)), and equal the oracle's where the oracle is cheap.

Frames of wimax_2304_0.5: the on-device source, seed 20260213, from frame 32768
on (the benchmark's first timed step), generated once.
"""
import numpy as np
import pytest
from scipy import sparse

import oracle
import synth_graphs as sg
from conftest import hstd_for
from db_codes import db_hstd
from parity_graphs import SHORT
from test_gpu_parity import _random_llr

pytestmark = pytest.mark.gpu

CODE = "wimax_2304_0.5"
SEED = 20260213
FRAME0 = 32768
_ALL = dict(nllr=True, post=True, hist=True, msgs=True)
_KEYS = ("z", "conv", "status", "iters", "nllr", "hist", "post", "msgs")
_LLR = {}
_DEC = {}


@pytest.fixture(autouse=True)
def _sub_tile_path_at_any_size(monkeypatch):
    """Small batches: keep the few-frame and column-parallel paths
    (LDPC_SMALL_COLS) away, so that tile_sub_kernel decodes them."""
    monkeypatch.setenv("LDPC_SMALL_COLS", "0")
    for var in ("LDPC_FIXED_POINT", "LDPC_FP_NEXT", "LDPC_PASS0_COLS", "LDPC_PASS0_LDS"):
        monkeypatch.delenv(var, raising=False)


@pytest.fixture(scope="module", autouse=True)
def _close_decoders():
    yield
    for dec in _DEC.values():
        dec.close()
    _DEC.clear()


def _decoder_for(key, H):
    """One 64-frame decoder per graph for the module; the graph must be on tile_sub_kernel's route."""
    from ldpc_amd import _lib
    from ldpc_amd.device import Decoder, Graph
    if key not in _DEC:
        g = Graph.cached(H)
        assert _lib.lib().ldpc_tile_kernel_name(g.handle).decode() == "tile_sub_kernel", key
        _DEC[key] = Decoder(g, 64)
    return _DEC[key]


def _decoder():
    return _decoder_for(CODE, hstd_for(CODE))


def _llr(dec, snr):
    """The 64 frames at `snr` dB: generated once, read-only."""
    if snr not in _LLR:
        _, llr = dec.generate(SEED, 0, oracle.sigma_for_snr(snr), FRAME0, 64)
        llr.setflags(write=False)
        _LLR[snr] = llr
    return _LLR[snr]


def _assert_identical(a, b, what):
    for key in _KEYS:
        assert a[key] is not None and b[key] is not None, key
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")


def _assert_oracle(H, r, llr, max_iter):
    assert max_iter <= 3 and len(llr) <= 32  # where the oracle is cheap
    o = oracle.spa_decode(H, llr, max_iter, nllr=True, want_L=False)
    for key in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(r[key][:len(llr)], o[key], err_msg=f"oracle: {key}")


def _lds_off(dec, llr, max_iter, monkeypatch):
    """The same decode with phase A gathering from global memory."""
    monkeypatch.setenv("LDPC_PASS0_LDS", "0")
    r = dec.decode(llr, max_iter, **_ALL)
    monkeypatch.delenv("LDPC_PASS0_LDS")
    return r


def _on_off_split(dec, llr, max_iter, monkeypatch, what=""):
    """decode() with the table in LDS (the default), with LDPC_PASS0_LDS=0 and
    by the split path; the three must agree."""
    on = dec.decode(llr, max_iter, **_ALL)
    _assert_identical(on, _lds_off(dec, llr, max_iter, monkeypatch), f"{what} T={max_iter} against LDPC_PASS0_LDS=0")
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(on, split, f"{what} T={max_iter} against the split path")
    return on


# ---- 1. switch on, switch off, split path, oracle
@pytest.mark.parametrize("max_iter", [1, 2])
def test_identical_with_the_switch_on_and_off_and_to_the_split_path(gpu_available, monkeypatch, max_iter):
    """48 frames at 1 dB (one tile, its fourth sub-tile empty).  T = 1 with the
    messages checks every E0 -- among them every identity-edge slot, which held
    its row's product before phase B wrote E0(r, k + r) over it."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:48]
    r = _on_off_split(dec, llr, max_iter, monkeypatch)
    assert (r.iters == max_iter).all()
    _assert_oracle(hstd_for(CODE), r, llr[:32], max_iter)


# ---- 2. a sub-tile that loses the vote next to sub-tiles in the column form
@pytest.mark.parametrize("max_iter", [2, 3])
def test_fallback_over_a_staged_table_next_to_the_column_form(gpu_available, monkeypatch, max_iter):
    """Frame 20 has ch = 0.0 in an A column: t = 0 in sub-tile 1's table, known
    only after the table is staged, so its row pipeline runs iteration 0 (rare
    rows) over an S region that held the table, and passes 1 and 2 sum into it.
    Sub-tiles 0 and 2 take the column form."""
    dec = _decoder()
    llr = np.array(_llr(dec, 1.0)[:48])
    llr[20, 100] = 0.0
    dec.rare_rows()  # reset
    sub = dec.decode(llr, max_iter, **_ALL)
    assert dec.rare_rows()[1] > 0
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(sub, split, f"T={max_iter} against the split path")
    _assert_identical(sub, _lds_off(dec, llr, max_iter, monkeypatch), f"T={max_iter} against LDPC_PASS0_LDS=0")
    dec.rare_rows()
    first = dec.decode(llr[:16], max_iter, **_ALL)
    assert dec.rare_rows()[1] == 0  # sub-tile 0 alone: the column form
    for key in _KEYS:
        np.testing.assert_array_equal(first[key], sub[key][:16], err_msg=f"T={max_iter} frames 0-15 alone: {key}")


# ---- 3. small shapes on this route
def _with_identity(A):
    m = A.shape[0]
    H = sparse.hstack([A, sparse.identity(m, dtype=np.int8, format="csr")], format="csr")
    H.sort_indices()
    return H


def _small_graph(name):
    """[A | I] graphs at k = 330 (past tile_kernel's LDS, no multiple of 64):
    m = 35 with a row that has its identity edge only, m = 38 with two empty A
    columns, m = k = 330, and m = 400 > k (P_r does not fit the S region: the
    row pipeline, nothing staged)."""
    if name == "idrow330":
        degs = sg._cycle(35, SHORT)
        degs[11] = 1
        return _with_identity(sg._deal(35, 330, [d - 1 for d in degs], 20261201))
    if name == "emptycol330":
        return _with_identity(sg._deal(38, 330, [d - 1 for d in sg._cycle(38, SHORT)], 20261202, empty=(0, 50)))
    if name == "m330k330":
        return _with_identity(sg._deal(330, 330, [d - 1 for d in sg._cycle(330, SHORT)], 20261203))
    assert name == "m400k330"
    return _with_identity(sg._deal(400, 330, [d - 1 for d in sg._cycle(400, (200, 233, 267, 300))], 20261204))


# graph -> (H, the two SNRs of its 8 + 8 frames)
_SHAPES = {
    "WRAN_N384_K320_R083": (lambda: db_hstd("WRAN_N384_K320_R083"), (1.0, 3.0)),   # m < k, k a multiple of 64
    "wigig_R05_N672_K336": (lambda: db_hstd("wigig_R05_N672_K336"), (1.5, 3.0)),   # m = k
    "idrow330": (lambda: _small_graph("idrow330"), (10.0, 13.0)),                  # m < k, neither a multiple of 64
    "emptycol330": (lambda: _small_graph("emptycol330"), (10.0, 13.0)),
    "m330k330": (lambda: _small_graph("m330k330"), (8.0, 11.0)),                   # m = k
    "m400k330": (lambda: _small_graph("m400k330"), (1.0, 4.0)),                    # m > k: the guard
}


@pytest.mark.parametrize("name", list(_SHAPES))
def test_small_shapes(gpu_available, monkeypatch, name):
    make, (lo, hi) = _SHAPES[name]
    H = sparse.csr_matrix(make())
    m, n = H.shape
    k = n - m
    deg = np.diff(H.indptr)
    cdeg = np.bincount(H.indices, minlength=n)
    if name == "idrow330":
        assert m < k and m % 64 and k % 64
        assert deg[11] == 1 and H.indices[H.indptr[11]] == k + 11  # reads nothing from LDS
    if name == "emptycol330":
        assert m < k and m % 64 and k % 64 and cdeg[0] == 0 and cdeg[50] == 0
    if name in ("m330k330", "wigig_R05_N672_K336"):
        assert m == k
    if name == "m400k330":
        assert m > k and 200 <= deg.min() and deg.max() <= 300
    dec = _decoder_for(name, H)  # asserts tile_sub_kernel
    idx = list(_SHAPES).index(name)
    llr = np.concatenate([_random_llr(H, 8, lo, 9300 + 2 * idx), _random_llr(H, 8, hi, 9301 + 2 * idx)])
    for max_iter in (1, 2):
        r = _on_off_split(dec, llr, max_iter, monkeypatch, name)
        _assert_oracle(H, r, llr, max_iter)


# ---- 4. frame-less lanes over a finished batch
def test_ragged_sub_tile_over_a_finished_batch(gpu_available, monkeypatch):
    """64 frames at 3 dB to T = 50, then 21 frames at 1 dB with T = 3 on the
    same decoder: sub-tile 1 has 5 live lanes and 11 frame-less ones over the
    L and E the first call left.  Frame-less lanes stage 1.0, hold no product
    in E and store nothing."""
    dec = _decoder()
    first = dec.decode(_llr(dec, 3.0), 50, post=True)
    assert first.post is not None
    llr = _llr(dec, 1.0)[:21]
    r = _on_off_split(dec, llr, 3, monkeypatch)
    _assert_oracle(hstd_for(CODE), r, llr, 3)


# ---- 5. exact bits through the holding place
def test_subnormal_and_zero_row_products(gpu_available, monkeypatch):
    """The 1 dB frames x 0.01, 16 frames, T = 2: a row's product of ~576 values
    near 0.025 is below 2^-900 and runs through the subnormals to zero, while no
    table value is tiny -- the products must come back from the holding place
    bit for bit."""
    dec = _decoder()
    H = hstd_for(CODE)
    llr = _llr(dec, 1.0)[:16] * 0.01
    t = np.tanh(np.clip(llr / 2, -17.5, 17.5))
    assert not (np.abs(t) <= 1e-10).any()
    log2p = (sparse.csr_matrix(H, dtype=np.float64) @ np.log2(np.abs(t)).T).T  # [frame, row]
    print("log2 |P_r|: min", log2p.min(), "max", log2p.max())
    assert (log2p < -900).any() and (log2p < -1100).any()
    r = _on_off_split(dec, llr, 2, monkeypatch)
    _assert_oracle(H, r, llr, 2)


def test_saturated_next_to_unscaled_frames(gpu_available, monkeypatch):
    """8 frames x 100 (t = +-CL nearly everywhere) next to 8 unscaled ones in
    one sub-tile, T = 2."""
    dec = _decoder()
    base = _llr(dec, 1.0)
    llr = np.concatenate([base[:8] * 100.0, base[8:16]])
    assert (np.abs(llr[:8]) / 2 > 17.5).mean() > 0.8
    r = _on_off_split(dec, llr, 2, monkeypatch)
    _assert_oracle(hstd_for(CODE), r, llr, 2)


# ---- 6. Monte-Carlo
def test_static_mc_run_with_the_switch_on_and_off(gpu_available, monkeypatch):
    """One static Monte-Carlo step of 64 frames at 1 dB, T = 50: equal counters
    and equal fixed-point counts."""
    dec = _decoder()
    sig = [oracle.sigma_for_snr(1.0)]
    dec.fixed_point()  # reset
    on = dec.mc_run(SEED, sig, 64, FRAME0, 50, nllr=True, static=True)
    fp_on = dec.fixed_point()
    monkeypatch.setenv("LDPC_PASS0_LDS", "0")
    off = dec.mc_run(SEED, sig, 64, FRAME0, 50, nllr=True, static=True)
    fp_off = dec.fixed_point()
    print("counters:", on.tolist(), "fixed_point:", fp_on, fp_off)
    assert on[0][0] == 64
    np.testing.assert_array_equal(on, off)
    assert fp_on == fp_off and fp_on[0] > 0
