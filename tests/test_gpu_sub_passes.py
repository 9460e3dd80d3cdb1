"""The passes of the static 16-frame sub-tile decoder (tile_sub_kernel<4>,
wimax_2304_0.5) that are not steady-state passes:

  pass 0          gathers t = tanh(clamp(ch/2)) from a per-column table that the
                  workgroup leaves in the tile's L, instead of evaluating tanh
                  once per edge;
  verifying pass  stores only the messages whose bits differ from the ones in
                  memory.

Both are exact, so every output -- hard bits, convergence iteration, Result,
iterations, normalized LLR and its history, posteriors, messages -- must be
IDENTICAL to the split path's (decode(..., split=True): per-iteration CN/VN
launches that share none of this code and are themselves held to the oracle),
and equal the oracle's where the oracle is cheap (T <= 3, <= 32 frames).

Frames: the on-device source, seed 20260213, from frame 32768 on (the
benchmark's first timed step).  Each set of frames is generated once.
"""
import numpy as np
import pytest

import oracle
from conftest import hstd_for

pytestmark = pytest.mark.gpu

CODE = "wimax_2304_0.5"
SEED = 20260213
FRAME0 = 32768
_ALL = dict(nllr=True, post=True, hist=True, msgs=True)
_KEYS = ("z", "conv", "status", "iters", "nllr", "hist", "post", "msgs")
_LLR = {}


@pytest.fixture(autouse=True)
def _sub_tile_path_at_any_size(monkeypatch):
    """Small batches: keep the few-frame and column-parallel paths
    (LDPC_SMALL_COLS) away, so that tile_sub_kernel decodes them."""
    monkeypatch.setenv("LDPC_SMALL_COLS", "0")
    monkeypatch.delenv("LDPC_FIXED_POINT", raising=False)


def _decoder(frames=64):
    from ldpc_amd.device import Decoder, Graph
    return Decoder(Graph.cached(hstd_for(CODE)), frames)


def _llr(dec, snr, test_zero=False):
    """The 64 frames at `snr` dB: generated once, read-only."""
    key = (snr, test_zero)
    if key not in _LLR:
        _, llr = dec.generate(SEED, 0, oracle.sigma_for_snr(snr), FRAME0, 64, test_zero=test_zero)
        llr.setflags(write=False)
        _LLR[key] = llr
    return _LLR[key]


def _assert_identical(a, b, what):
    for key in _KEYS:
        assert a[key] is not None and b[key] is not None, key
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")


def _assert_oracle(r, llr, max_iter):
    assert max_iter <= 3 and len(llr) <= 32  # where the oracle is cheap
    o = oracle.spa_decode(hstd_for(CODE), llr, max_iter, nllr=True, want_L=False)
    for key in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(r[key][:len(llr)], o[key], err_msg=f"oracle: {key}")


def _sub_and_split(dec, llr, max_iter):
    """decode() by tile_sub_kernel, then by the split path; the two must agree."""
    sub = dec.decode(llr, max_iter, **_ALL)
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(sub, split, f"T={max_iter} against the split path")
    return sub


@pytest.mark.parametrize("max_iter", [1, 2])
def test_pass0_alone_and_its_hand_over(gpu_available, max_iter):
    """48 frames at 1 dB (one tile, its fourth sub-tile empty): T = 1 is pass 0
    alone, T = 2 hands its messages and posteriors to a normal pass."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:48]
    r = _sub_and_split(dec, llr, max_iter)
    assert (r.iters == max_iter).all()
    _assert_oracle(r, llr[:32], max_iter)


@pytest.mark.parametrize("max_iter", [1, 2])
def test_pass0_rare_rows_from_table_values(gpu_available, max_iter):
    """32 frames with the frame source's erasures: ch = 0 gives t = 0, so the
    |t| <= 1e-10 vote of pass 0 is taken on table values."""
    dec = _decoder()
    llr = _llr(dec, 1.0, test_zero=True)[:32]
    assert (llr == 0.0).any()
    dec.rare_rows()  # reset
    sub = dec.decode(llr, max_iter, **_ALL)
    assert dec.rare_rows()[1] > 0
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(sub, split, f"T={max_iter} against the split path")
    _assert_oracle(sub, llr, max_iter)


def test_pass0_saturated_and_mixed_llrs(gpu_available):
    """The 1 dB frames scaled by 100, 16 frames, T = 2: most |ch|/2 are past
    the +-17.5 clamp (t = +-1 exactly), the rest are not."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:16] * 100.0
    half = np.abs(llr) / 2
    assert (half > 17.5).any() and (half < 17.5).any()
    r = _sub_and_split(dec, llr, 2)
    _assert_oracle(r, llr, 2)


def test_ragged_sub_tile_over_a_finished_batch(gpu_available):
    """64 frames at 3 dB to T = 50, then 20 frames at 1 dB with T = 3 on the
    same decoder: sub-tile 1 has 4 live lanes and 12 frame-less ones over the
    state the first call left (their L must not take the pass-0 table, and
    what they gather from it must not reach a live frame)."""
    dec = _decoder()
    first = dec.decode(_llr(dec, 3.0), 50, post=True)
    assert first.post is not None
    llr = _llr(dec, 1.0)[:20]
    r = _sub_and_split(dec, llr, 3)
    _assert_oracle(r, llr, 3)


@pytest.mark.parametrize("max_iter", [3, 4, 6, 10])
def test_partial_confirmation(gpu_available, monkeypatch, max_iter):
    """64 frames at 2 dB (a mixed workgroup), outputs taken right after a
    verifying pass that confirmed only some frames of a sub-tile (T = 3, 4:
    the first one, at iteration 2) and a few passes later: the messages that
    differed must have been stored."""
    dec = _decoder()
    llr = _llr(dec, 2.0)
    dec.fixed_point()  # reset
    on = _sub_and_split(dec, llr, max_iter)
    print("fixed_point:", dec.fixed_point())
    monkeypatch.setenv("LDPC_FIXED_POINT", "0")
    off = dec.decode(llr, max_iter, **_ALL)
    assert dec.fixed_point() == (0, 0)
    _assert_identical(on, off, f"T={max_iter} against LDPC_FIXED_POINT=0")


def test_headline_frames_at_t50(gpu_available, monkeypatch):
    """48 frames at 1 dB, T = 50, exit on: every frame stops after the
    verifying pass at iteration 2, as before the change (48 frames, 47 passes
    skipped each), and nothing differs from a run with the exit off."""
    dec = _decoder()
    llr = _llr(dec, 1.0)[:48]
    dec.fixed_point()  # reset
    on = dec.decode(llr, 50, **_ALL)
    fp = dec.fixed_point()
    print("fixed_point:", fp)
    assert fp == (48, 48 * 47)
    split = dec.decode(llr, 50, split=True, **_ALL)
    _assert_identical(on, split, "T=50 against the split path")
    monkeypatch.setenv("LDPC_FIXED_POINT", "0")
    off = dec.decode(llr, 50, **_ALL)
    assert dec.fixed_point() == (0, 0)
    _assert_identical(on, off, "T=50 against LDPC_FIXED_POINT=0")
