"""The fixed-point exit of the static 16-frame sub-tile decoder
(tile_sub_kernel<4>, wimax_2304_0.5): a frame whose pass reproduced its
messages and posteriors bit for bit stops there with the outputs of pass
max_iter.  The exit is exact, so every output -- hard bits, convergence
iteration, Result, iterations, normalized LLR and its history, posteriors,
messages -- must be IDENTICAL with the exit on and under LDPC_FIXED_POINT=0,
and equal the oracle's where that is compared.

Frames: the on-device source, seed 20260213, from frame 32768 on (the
benchmark's first timed step).  The oracle decodes the 64 frames at 1 dB once
for the tests that need it.
"""
import numpy as np
import pytest

import oracle
from conftest import hstd_for

pytestmark = pytest.mark.gpu

CODE = "wimax_2304_0.5"
SEED = 20260213
FRAME0 = 32768
T = 50
_ORACLE = {}


@pytest.fixture(autouse=True)
def _sub_tile_path_at_any_size(monkeypatch):
    """Small batches: keep the few-frame and column-parallel paths
    (LDPC_SMALL_COLS) away, so that tile_sub_kernel decodes them."""
    monkeypatch.setenv("LDPC_SMALL_COLS", "0")
    monkeypatch.delenv("LDPC_FIXED_POINT", raising=False)


def _decoder(frames=64):
    from ldpc_amd.device import Decoder, Graph
    return Decoder(Graph.cached(hstd_for(CODE)), frames)


def _frames(dec, snr, count, test_zero=False):
    return dec.generate(SEED, 0, oracle.sigma_for_snr(snr), FRAME0, count, test_zero=test_zero)


def _oracle_1db(dec):
    """(u, llr, oracle outputs) of the 64 frames at 1 dB, T = 50: computed once."""
    if "1db" not in _ORACLE:
        u, llr = _frames(dec, 1.0, 64)
        _ORACLE["1db"] = (u, llr, oracle.spa_decode(hstd_for(CODE), llr, T, nllr=True, want_L=False))
    return _ORACLE["1db"]


def _both(dec, monkeypatch, llr, max_iter, **kw):
    """decode() with the exit on and off; returns (on, counters of the on run, off)."""
    dec.fixed_point()  # reset
    on = dec.decode(llr, max_iter, **kw)
    fp = dec.fixed_point()
    monkeypatch.setenv("LDPC_FIXED_POINT", "0")
    off = dec.decode(llr, max_iter, **kw)
    assert dec.fixed_point() == (0, 0)
    monkeypatch.delenv("LDPC_FIXED_POINT")
    return on, fp, off


def _assert_identical(a, b):
    for key in ("z", "conv", "status", "iters", "nllr", "hist", "post", "msgs"):
        va, vb = getattr(a, key), getattr(b, key)
        assert (va is None) == (vb is None), key
        if va is not None:
            np.testing.assert_array_equal(va, vb, err_msg=key)


def _assert_oracle(r, o, rows=slice(None)):
    for key in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(r[key], o[key][rows], err_msg=key)


_ALL = dict(nllr=True, post=True, hist=True, msgs=True)


def test_headline_frames_stop_after_a_few_passes(gpu_available, monkeypatch):
    """48 frames at 1 dB (one tile, its fourth sub-tile empty): every frame
    fails and sits at a fixed point after 3 passes on the oracle."""
    dec = _decoder()
    _, llr, o = _oracle_1db(dec)
    on, fp, off = _both(dec, monkeypatch, llr[:48], T, **_ALL)
    _assert_identical(on, off)
    _assert_oracle(on, o, slice(0, 48))
    assert (on.status == 1).all() and (on.iters == T).all()
    print("fixed_point:", fp)
    assert fp[0] == 48
    assert fp[1] > 48 * 40


def test_mixed_workgroup_at_2db(gpu_available, monkeypatch):
    """64 frames at 2 dB: frames of one workgroup converge, stop at a fixed
    point at different passes, or never settle."""
    dec = _decoder()
    _, llr = _frames(dec, 2.0, 64)
    on, fp, off = _both(dec, monkeypatch, llr, T, **_ALL)
    _assert_identical(on, off)
    print("fixed_point:", fp, "converged:", int((on.status == 0).sum()))
    assert 0 < fp[0] < 64


def test_rare_rows_on_every_pass(gpu_available, monkeypatch):
    """32 frames at 1 dB with the frame source's erasures: rare rows
    (|t| <= 1e-10) on every pass, the verifying one included."""
    dec = _decoder()
    _, llr = _frames(dec, 1.0, 32, test_zero=True)
    assert (llr == 0.0).any()
    dec.rare_rows()  # reset
    on, fp, off = _both(dec, monkeypatch, llr, T, **_ALL)
    assert dec.rare_rows()[1] > 0
    _assert_identical(on, off)
    print("fixed_point:", fp)
    _assert_oracle(on, oracle.spa_decode(hstd_for(CODE), llr, T, nllr=True, want_L=False))


@pytest.mark.parametrize("max_iter", [1, 2, 3, 4])
def test_short_runs_make_every_pass(gpu_available, monkeypatch, max_iter):
    """T = 1 .. 4 at 1 dB: the exit cannot fire before a verifying pass exists
    (iteration >= 1, after a pass whose posteriors repeated)."""
    dec = _decoder()
    _, llr, _ = _oracle_1db(dec)
    on, fp, off = _both(dec, monkeypatch, llr[:16], max_iter, **_ALL)
    _assert_identical(on, off)
    assert (on.iters == max_iter).all()
    print("fixed_point:", fp)
    if max_iter <= 2:  # passes 0 and 1 can trigger, neither can verify
        assert fp == (0, 0)


def test_static_mc_counters(gpu_available, monkeypatch):
    """mc_run(static=True) over the 64 frames at 1 dB == the split path == the oracle."""
    dec = _decoder()
    u, _, o = _oracle_1db(dec)
    sig = [oracle.sigma_for_snr(1.0)]
    dec.fixed_point()  # reset
    a = dec.mc_run(SEED, sig, 64, FRAME0, T, nllr=True, static=True)
    fp = dec.fixed_point()
    b = dec.mc_run(SEED, sig, 64, FRAME0, T, nllr=True, static=True, split=True)
    assert dec.fixed_point() == (0, 0)  # the split path has no such exit
    np.testing.assert_array_equal(a, b)
    k = u.shape[1]
    want = oracle.main_counters(u, o["z"], o["status"], o["conv"], nllr_cnt=np.rint(o["nllr"] * k), iters=o["iters"])
    np.testing.assert_array_equal(a[0], want)
    print("fixed_point:", fp)
    assert fp[0] > 0
