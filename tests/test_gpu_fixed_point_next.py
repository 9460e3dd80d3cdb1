"""The next-pass proof in the fixed-point exit of the static 16-frame sub-tile
decoder (tile_sub_kernel<4>, wimax_2304_0.5): a verifying pass whose messages
differed still stops a frame when it proves that the next pass would form the
same variable-to-check values (tile_sub.hip "Fixed-point exit";
test_fixed_point_proof.py checks the proof itself on the CPU).  The exit stays
exact, so every output -- hard bits, convergence iteration, Result, iterations,
normalized LLR and its history, posteriors, messages -- must be IDENTICAL with
the proof (the default), without it (LDPC_FP_NEXT=0), with the exit off
(LDPC_FIXED_POINT=0) and on the split path, and the counts of
Decoder.fixed_point() must be the ones that the restated schedule
(fixed_point_ref.py) gives from the GPU's own exit-off states after passes
0 .. 4 (at 2 dB 0 .. 9, and 0 .. 49 in a longer test).

Frames: the on-device source, seed 20260213.  Frames 32768 + 130, + 256 and
+ 262 at 1 dB are stragglers: their posteriors repeat in pass 2 and their
messages do not, so that without the proof their sub-tile runs a 4th pass.
"""
import numpy as np
import pytest

import fixed_point_ref as ref
import oracle
from conftest import hstd_for

pytestmark = pytest.mark.gpu

CODE = "wimax_2304_0.5"
SEED = 20260213
FRAME0 = 32768
T = 50
_ALL = dict(nllr=True, post=True, hist=True, msgs=True)
_KEYS = ("z", "conv", "status", "iters", "nllr", "hist", "post", "msgs")


@pytest.fixture(autouse=True)
def _sub_tile_path_at_any_size(monkeypatch):
    """Small batches: keep the few-frame and column-parallel paths
    (LDPC_SMALL_COLS) away, so that tile_sub_kernel decodes them."""
    monkeypatch.setenv("LDPC_SMALL_COLS", "0")
    monkeypatch.delenv("LDPC_FIXED_POINT", raising=False)
    monkeypatch.delenv("LDPC_FP_NEXT", raising=False)


def _decoder(frames=64):
    from ldpc_amd.device import Decoder, Graph
    return Decoder(Graph.cached(hstd_for(CODE)), frames)


def _frames(dec, snr, offset, count, test_zero=False):
    return dec.generate(SEED, 0, oracle.sigma_for_snr(snr), FRAME0 + offset, count, test_zero=test_zero)


def _assert_identical(a, b, what):
    for key in _KEYS:
        assert a[key] is not None and b[key] is not None, key
        np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")


def _run(dec, monkeypatch, llr, max_iter, **env):
    """decode() under the environment given; returns (outputs, fixed_point())."""
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    dec.fixed_point()  # reset
    r = dec.decode(llr, max_iter, **_ALL)
    fp = dec.fixed_point()
    for name in env:
        monkeypatch.delenv(name)
    return r, fp


def _restated(dec, monkeypatch, llr, max_iter, passes=5):
    """fixed_point() pairs (with the proof, without it) of the restated
    schedule, from the GPU's exit-off states after passes 0 .. passes - 1."""
    monkeypatch.setenv("LDPC_FIXED_POINT", "0")
    states = [dec.decode(llr, p + 1, post=True, msgs=True) for p in range(passes)]
    monkeypatch.delenv("LDPC_FIXED_POINT")
    g = dec.graph
    pd, md, nx = ref.flags(llr, states, g.indices, g.k)
    conv = states[-1]["conv"]
    return [ref.replay(pd, md, nx, conv, max_iter, next_rule=rule) for rule in (True, False)], (pd, md, nx)


def _all_ways(dec, monkeypatch, llr, max_iter):
    on, fp_on = _run(dec, monkeypatch, llr, max_iter)
    par, fp_par = _run(dec, monkeypatch, llr, max_iter, LDPC_FP_NEXT="0")
    off, fp_off = _run(dec, monkeypatch, llr, max_iter, LDPC_FIXED_POINT="0")
    assert fp_off == (0, 0)
    split = dec.decode(llr, max_iter, split=True, **_ALL)
    _assert_identical(on, off, f"T={max_iter} against LDPC_FIXED_POINT=0")
    _assert_identical(par, off, f"T={max_iter}, LDPC_FP_NEXT=0 against LDPC_FIXED_POINT=0")
    _assert_identical(on, split, f"T={max_iter} against the split path")
    return on, fp_on, fp_par


@pytest.mark.parametrize("offset,count,stragglers", [(128, 32, (2,)), (256, 16, (0, 6))])
def test_stragglers_stop_with_their_sub_tile(gpu_available, monkeypatch, offset, count, stragglers):
    """32 frames from 32768 + 128 (sub-tile 0 holds straggler 130, sub-tile 1
    none) and 16 frames from 32768 + 256 (two stragglers in one sub-tile)."""
    dec = _decoder()
    _, llr = _frames(dec, 1.0, offset, count)
    on, fp_on, fp_par = _all_ways(dec, monkeypatch, llr, T)
    (want_on, want_par), (pd, md, nx) = _restated(dec, monkeypatch, llr, T)
    print("fixed_point:", fp_on, "LDPC_FP_NEXT=0:", fp_par, "restated:", want_on[0], want_par[0])
    for f in stragglers:  # on the GPU's own bits
        assert not pd[2, f] and md[2, f] and not nx[2, f], f
    assert fp_on == want_on[0]
    assert fp_par == want_par[0]
    assert fp_on[1] > fp_par[1]
    assert fp_on == (count, count * (T - 3))  # every frame stops after three passes
    assert (on.status == 1).all() and (on.iters == T).all()


@pytest.mark.parametrize("max_iter", [3, 4])
def test_right_after_a_proof_based_stop(gpu_available, monkeypatch, max_iter):
    """The 16-frame case at T = 3 and T = 4: outputs taken right after the
    verifying pass at iteration 2 and one pass later -- the messages that
    differed in the pass that proved the stop must have been stored."""
    dec = _decoder()
    _, llr = _frames(dec, 1.0, 256, 16)
    on, fp_on, fp_par = _all_ways(dec, monkeypatch, llr, max_iter)
    print("fixed_point:", fp_on, "LDPC_FP_NEXT=0:", fp_par)
    assert (on.iters == max_iter).all()
    if max_iter == 4:  # at T = 3 iteration 2 is the max-iteration exit
        assert fp_on == (16, 16) and fp_par[0] < 16


def test_mixed_workgroup_at_2db(gpu_available, monkeypatch):
    """64 frames at 2 dB: frames of one workgroup converge, stop at a fixed
    point at different passes, or never settle.  T = 50 against the exit off;
    the counts against the restated schedule at T = 10, where the first frames
    have stopped (test_mixed_workgroup_counts_at_t50: the same at T = 50)."""
    dec = _decoder()
    _, llr = _frames(dec, 2.0, 0, 64)
    on, fp_on = _run(dec, monkeypatch, llr, T)
    off, fp_off = _run(dec, monkeypatch, llr, T, LDPC_FIXED_POINT="0")
    assert fp_off == (0, 0)
    _assert_identical(on, off, "T=50 against LDPC_FIXED_POINT=0")
    print("fixed_point at T=50:", fp_on, "converged:", int((on.status == 0).sum()))
    assert 0 < fp_on[0] < 64
    short, fp_short = _run(dec, monkeypatch, llr, 10)
    par, fp_par = _run(dec, monkeypatch, llr, 10, LDPC_FP_NEXT="0")
    (want_on, want_par), _ = _restated(dec, monkeypatch, llr, 10, passes=10)
    print("fixed_point at T=10:", fp_short, "LDPC_FP_NEXT=0:", fp_par, "restated:", want_on[0], want_par[0])
    _assert_identical(short, par, "T=10 against LDPC_FP_NEXT=0")
    assert fp_short == want_on[0]
    assert fp_par == want_par[0]


def test_mixed_workgroup_counts_at_t50(gpu_available, monkeypatch):
    """The same 64 frames at 2 dB, T = 50: the counts with the proof and
    without it equal the restated schedule's, over every back-off of the 50
    passes.  The restatement takes the exit-off posteriors after each of the
    50 passes (each a decode from the start: this test takes tens of seconds)
    and the messages only of the passes in which some sub-tile verifies."""
    dec = _decoder()
    g = dec.graph
    _, llr = _frames(dec, 2.0, 0, 64)
    _, fp_on = _run(dec, monkeypatch, llr, T)
    _, fp_par = _run(dec, monkeypatch, llr, T, LDPC_FP_NEXT="0")
    monkeypatch.setenv("LDPC_FIXED_POINT", "0")
    pd = np.ones((T, 64), bool)
    prev = llr
    for p in range(T):
        r = dec.decode(llr, p + 1, post=True)
        pd[p] = (ref._bits(r.post[:, :g.k]) != ref._bits(prev[:, :g.k])).any(axis=1)
        prev, conv = r.post, r.conv
    state, done = {}, {}

    def _state(t):  # after t passes; the last two asked for are kept
        if t not in state:
            for old in [o for o in state if o < t - 1]:
                del state[old]
            state[t] = dec.decode(llr, t, post=True, msgs=True)
        return state[t]

    def lazy(it):
        if it not in done:
            done[it] = ref.pass_flags(_state(it), _state(it + 1), g.indices, g.k)
        return done[it]

    want_on, _ = ref.replay(pd, None, None, conv, T, next_rule=True, lazy=lazy)
    want_par, _ = ref.replay(pd, None, None, conv, T, next_rule=False, lazy=lazy)
    monkeypatch.delenv("LDPC_FIXED_POINT")
    print("fixed_point at T=50:", fp_on, "LDPC_FP_NEXT=0:", fp_par, "restated:", want_on, want_par,
          "verifying passes:", sorted(done))
    assert fp_on == want_on
    assert fp_par == want_par


def test_rare_rows_on_the_verifying_passes(gpu_available, monkeypatch):
    """32 frames at 1 dB with the frame source's erasures: rare rows
    (|t| <= 1e-10) on every pass, the verifying ones included."""
    dec = _decoder()
    _, llr = _frames(dec, 1.0, 0, 32, test_zero=True)
    assert (llr == 0.0).any()
    dec.rare_rows()  # reset
    on, fp_on = _run(dec, monkeypatch, llr, T)
    assert dec.rare_rows()[1] > 0
    off, fp_off = _run(dec, monkeypatch, llr, T, LDPC_FIXED_POINT="0")
    assert fp_off == (0, 0)
    _assert_identical(on, off, "T=50 against LDPC_FIXED_POINT=0")
    print("fixed_point:", fp_on)
    o = oracle.spa_decode(hstd_for(CODE), llr, T, nllr=True, want_L=False)
    for key in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(on[key], o[key], err_msg=f"oracle: {key}")


def test_ragged_sub_tile_over_a_finished_batch(gpu_available, monkeypatch):
    """64 frames at 3 dB to T = 50, then 20 frames at 1 dB from 32768 + 256 on
    the same decoder: sub-tile 0 holds the two stragglers, sub-tile 1 has 4
    live lanes and 12 frame-less ones over the state the first call left.
    Frame-less lanes must neither vote nor stop: the counts are those of the
    20 frames."""
    dec = _decoder()
    _, first = _frames(dec, 3.0, 0, 64)
    assert dec.decode(first, T, post=True).post is not None
    _, llr = _frames(dec, 1.0, 256, 20)
    on, fp_on, fp_par = _all_ways(dec, monkeypatch, llr, T)
    (want_on, want_par), _ = _restated(dec, monkeypatch, llr, T)
    print("fixed_point:", fp_on, "LDPC_FP_NEXT=0:", fp_par)
    assert fp_on == want_on[0] == (20, 20 * (T - 3))
    assert fp_par == want_par[0]
    assert fp_on[1] > fp_par[1]


def test_static_mc_counters(gpu_available, monkeypatch):
    """mc_run(static=True) over 64 frames from 32768 + 256 == the split path == the oracle."""
    dec = _decoder()
    sig = [oracle.sigma_for_snr(1.0)]
    dec.fixed_point()  # reset
    a = dec.mc_run(SEED, sig, 64, FRAME0 + 256, T, nllr=True, static=True)
    fp = dec.fixed_point()
    b = dec.mc_run(SEED, sig, 64, FRAME0 + 256, T, nllr=True, static=True, split=True)
    assert dec.fixed_point() == (0, 0)  # the split path has no such exit
    np.testing.assert_array_equal(a, b)
    u, llr = _frames(dec, 1.0, 256, 64)
    o = oracle.spa_decode(hstd_for(CODE), llr, T, nllr=True, want_L=False)
    k = u.shape[1]
    want = oracle.main_counters(u, o["z"], o["status"], o["conv"], nllr_cnt=np.rint(o["nllr"] * k), iters=o["iters"])
    np.testing.assert_array_equal(a[0], want)
    print("fixed_point:", fp)
    assert fp[0] == 64
