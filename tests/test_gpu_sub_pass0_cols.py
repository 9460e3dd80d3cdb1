"""Iteration 0 of the static 16-frame sub-tile decoder (tile_sub_kernel<4>) in
its column form (tile_sub.hip sub_pass0_cols): row products by independent
lanes, then every column's messages, sum and posterior by one lane group, with
no row chain.  LDPC_PASS0_COLS=0 keeps the row pipeline for iteration 0; a
sub-tile with a table value |t| <= 1e-10 and a graph with m > k run it too.

The form is exact, so every output -- hard bits, convergence iteration, Result,
iterations, normalized LLR and its history, posteriors, messages -- must be
IDENTICAL to the split path's (decode(..., split=True)) and to the row
pipeline's, and equal the oracle's where the oracle is cheap.

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
    monkeypatch.delenv("LDPC_FIXED_POINT", raising=False)
    monkeypatch.delenv("LDPC_PASS0_COLS", raising=False)


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


def _sub_and_split(dec, llr, max_iter):
    """decode() by tile_sub_kernel, then by the split path; the two must agree."""
    sub = dec.decode(llr, max_iter, **_ALL)
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(sub, split, f"T={max_iter} against the split path")
    return sub


def _rows_off(dec, llr, max_iter, monkeypatch):
    """The same decode with iteration 0 by the row pipeline."""
    monkeypatch.setenv("LDPC_PASS0_COLS", "0")
    r = dec.decode(llr, max_iter, **_ALL)
    monkeypatch.delenv("LDPC_PASS0_COLS")
    return r


# ---- 1. identity with the split path and with the row pipeline's iteration 0
@pytest.mark.parametrize("max_iter", [1, 2])
def test_identical_to_split_path_and_row_pipeline(gpu_available, monkeypatch, max_iter):
    """48 frames at 1 dB (one tile, its fourth sub-tile empty).  T = 1 with the
    messages is the direct check of every E0, its CSR position and every L."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:48]
    r = _sub_and_split(dec, llr, max_iter)
    assert (r.iters == max_iter).all()
    _assert_identical(r, _rows_off(dec, llr, max_iter, monkeypatch), f"T={max_iter} against LDPC_PASS0_COLS=0")
    _assert_oracle(hstd_for(CODE), r, llr[:32], max_iter)


# ---- 2. the row pipeline (a tiny table value) and the column form in one tile
def test_fallback_and_column_form_in_one_tile(gpu_available):
    """Frames 0-15 untouched (sub-tile 0: the column form); frame 20 with
    ch = 0.0 in an A column and frame 40 in an identity column (sub-tiles 1 and
    2: t = 0 in the table, so the row pipeline and its rare rows)."""
    dec = _decoder()
    H = hstd_for(CODE)
    k = H.shape[1] - H.shape[0]
    llr = np.array(_llr(dec, 1.0)[:48])
    llr[20, 100] = 0.0
    llr[40, k + 7] = 0.0
    for max_iter in (1, 2, 3):
        dec.rare_rows()  # reset
        sub = dec.decode(llr, max_iter, **_ALL)
        assert dec.rare_rows()[1] > 0
        split = dec.decode(llr, max_iter, split=True, **_ALL)
        _assert_identical(sub, split, f"T={max_iter} against the split path")
        dec.rare_rows()
        first = dec.decode(llr[:16], max_iter, **_ALL)
        assert dec.rare_rows()[1] == 0
        for key in _KEYS:
            np.testing.assert_array_equal(first[key], sub[key][:16], err_msg=f"T={max_iter} frames 0-15 alone: {key}")


# ---- 3. large quotients: the clip and atanh
def test_saturated_llrs_take_atanh_in_every_step(gpu_available, monkeypatch):
    """The 1 dB frames x 100, 16 frames, T = 2.  Frames whose |ch|/2 all pass
    the +-17.5 clamp have t = +-CL everywhere; q = P/t is then far from 2^-27
    in every wavefront step."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:16] * 100.0
    assert (np.abs(llr) / 2 > 17.5).mean() > 0.8
    r = _sub_and_split(dec, llr, 2)
    _assert_identical(r, _rows_off(dec, llr, 2, monkeypatch), "against LDPC_PASS0_COLS=0")
    _assert_oracle(hstd_for(CODE), r, llr, 2)


def test_saturated_next_to_unscaled_frames(gpu_available, monkeypatch):
    """8 such frames next to 8 unscaled ones in one sub-tile: the 2q / atanh
    vote is mixed within a wavefront step."""
    dec = _decoder()
    base = _llr(dec, 1.0)
    llr = np.concatenate([base[:8] * 100.0, base[8:16]])
    r = _sub_and_split(dec, llr, 2)
    _assert_identical(r, _rows_off(dec, llr, 2, monkeypatch), "against LDPC_PASS0_COLS=0")
    _assert_oracle(hstd_for(CODE), r, llr, 2)


# ---- 4. small products: div_nr_ok false, subnormal and zero P
def test_row_products_below_the_division_shortcut(gpu_available, monkeypatch):
    """The 1 dB frames x 0.01, 16 frames, T = 2: a row's product of ~576 values
    near 0.025 is below 2^-900 (and below the subnormals), while no table value
    is tiny -- the column form is the path under test."""
    dec = _decoder()
    H = hstd_for(CODE)
    llr = _llr(dec, 1.0)[:16] * 0.01
    t = np.tanh(np.clip(llr / 2, -17.5, 17.5))
    assert not (np.abs(t) <= 1e-10).any()
    log2p = (sparse.csr_matrix(H, dtype=np.float64) @ np.log2(np.abs(t)).T).T  # [frame, row]
    print("log2 |P_r|: min", log2p.min(), "max", log2p.max())
    assert (log2p < -900).any() and (log2p < -1100).any()
    r = _sub_and_split(dec, llr, 2)
    _assert_identical(r, _rows_off(dec, llr, 2, monkeypatch), "against LDPC_PASS0_COLS=0")
    _assert_oracle(H, r, llr, 2)


# ---- 5. a ragged sub-tile over a finished batch
def test_ragged_sub_tile_over_a_finished_batch(gpu_available):
    """64 frames at 3 dB to T = 50, then 20 frames at 1 dB with T = 3 on the
    same decoder: sub-tile 1 has 4 live lanes and 12 frame-less ones over the
    state the first call left.  Frame-less lanes store nothing and their L does
    not take the table."""
    dec = _decoder()
    first = dec.decode(_llr(dec, 3.0), 50, post=True)
    assert first.post is not None
    llr = _llr(dec, 1.0)[:20]
    r = _sub_and_split(dec, llr, 3)
    _assert_oracle(hstd_for(CODE), r, llr, 3)


# ---- 6. other shapes on this route
def _with_identity(A):
    m = A.shape[0]
    H = sparse.hstack([A, sparse.identity(m, dtype=np.int8, format="csr")], format="csr")
    H.sort_indices()
    return H


def _limit_graph(name):
    """The limit graphs of parity_graphs.py with an identity-only row and with
    empty columns, at k = 320, where tile_kernel's LDS is out and the sub-tile
    decoder runs; and an [A | I] graph with m > k (P_r does not fit the S
    region: the row pipeline)."""
    if name == "idrow320":
        degs = sg._cycle(35, SHORT)
        degs[11] = 1
        return _with_identity(sg._deal(35, 320, [d - 1 for d in degs], 20261101))
    if name == "emptycol320":
        return _with_identity(sg._deal(38, 320, [d - 1 for d in sg._cycle(38, SHORT)], 20261102, empty=(0, 50)))
    assert name == "m400k320"
    return _with_identity(sg._deal(400, 320, [d - 1 for d in sg._cycle(400, (200, 233, 267, 300))], 20261103))


# graph -> (H, the two SNRs of its 8 + 8 frames)
_SHAPES = {
    "WRAN_N384_K320_R083": (lambda: db_hstd("WRAN_N384_K320_R083"), (1.0, 3.0)),   # m < k
    "wigig_R05_N672_K336": (lambda: db_hstd("wigig_R05_N672_K336"), (1.5, 3.0)),   # m = k
    "idrow320": (lambda: _limit_graph("idrow320"), (10.0, 13.0)),
    "emptycol320": (lambda: _limit_graph("emptycol320"), (10.0, 13.0)),
    "m400k320": (lambda: _limit_graph("m400k320"), (1.0, 4.0)),                    # m > k: the guard
}


@pytest.mark.parametrize("name", list(_SHAPES))
def test_other_shapes(gpu_available, monkeypatch, name):
    make, (lo, hi) = _SHAPES[name]
    H = sparse.csr_matrix(make())
    m, n = H.shape
    deg = np.diff(H.indptr)
    cdeg = np.bincount(H.indices, minlength=n)
    if name == "idrow320":
        assert deg[11] == 1 and H.indices[H.indptr[11]] == n - m + 11
    if name == "emptycol320":
        assert cdeg[0] == 0 and cdeg[50] == 0
    if name == "m400k320":
        assert m > n - m and 200 <= deg.min() and deg.max() <= 300
    dec = _decoder_for(name, H)  # asserts tile_sub_kernel
    idx = list(_SHAPES).index(name)
    llr = np.concatenate([_random_llr(H, 8, lo, 9100 + 2 * idx), _random_llr(H, 8, hi, 9101 + 2 * idx)])
    for max_iter in (1, 2):
        r = _sub_and_split(dec, llr, max_iter)
        _assert_identical(r, _rows_off(dec, llr, max_iter, monkeypatch), f"{name} T={max_iter} against LDPC_PASS0_COLS=0")
        _assert_oracle(H, r, llr, max_iter)


# ---- 7. the pins of the fixed-point exit
def test_headline_frames_at_t50_with_the_switch_on_and_off(gpu_available, monkeypatch):
    """48 frames at 1 dB, T = 50: every frame stops after the verifying pass at
    iteration 2 (48 frames, 47 passes skipped each) whichever form iteration 0
    takes, and the outputs are identical."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:48]
    dec.fixed_point()  # reset
    on = dec.decode(llr, 50, **_ALL)
    fp_on = dec.fixed_point()
    monkeypatch.setenv("LDPC_PASS0_COLS", "0")
    off = dec.decode(llr, 50, **_ALL)
    fp_off = dec.fixed_point()
    print("fixed_point:", fp_on, fp_off)
    assert fp_on == (48, 48 * 47)
    assert fp_off == (48, 48 * 47)
    _assert_identical(on, off, "T=50 against LDPC_PASS0_COLS=0")


def test_static_mc_run_counters_with_the_switch_on_and_off(gpu_available, monkeypatch):
    """One static Monte-Carlo step of 64 frames at 1 dB, T = 50: equal counters."""
    dec = _decoder()
    sig = [oracle.sigma_for_snr(1.0)]
    on = dec.mc_run(SEED, sig, 64, FRAME0, 50, nllr=True, static=True)
    monkeypatch.setenv("LDPC_PASS0_COLS", "0")
    off = dec.mc_run(SEED, sig, 64, FRAME0, 50, nllr=True, static=True)
    print("counters:", on.tolist())
    assert on[0][0] == 64
    np.testing.assert_array_equal(on, off)
