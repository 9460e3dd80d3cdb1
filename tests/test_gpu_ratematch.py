"""The physical-mode frame source under a rate-matching pattern
(ldpc_rate_match_set: punctured and shortened columns) on the GPU.

1. generate() against the numpy restatement (tests/ratematch_ref.py: shortened
   info bits cleared, re-encoded from H, the compacted transmitted bits through
   tests/channel_ref.py, scattered back), for every channel spec on
   wimax_576_0.5 and the IRA graph, and on tiny graphs with an odd E, the first
   and last columns not sent and a symbol across k and a punctured run;
2. the three output forms carry the same frames: the Monte-Carlo counters of
   every decoder path equal the restatements' on the frames generate() returns;
3. mc.simulate with rate_match, and the failed-frame records;
4. nothing moved, nothing stale: no pattern / A / cleared / B / cleared on one
   decoder;
5. the refusals.
"""
import functools

import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import oracle
import qminsum_ref
import ratematch_ref
from conftest import hstd_for
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
from ldpc_amd.ratematch import KNOWN_LLR, RateMatch
from test_gpu_channel import ALL_SPECS, GEN_SIGMA, _graph_h, _id

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
W576 = "wimax_576_0.5"

# wimax_576_0.5 (k = 288): every sixth parity column punctured, the first 24 info bits shortened; E = 504
RM_W576 = RateMatch(tuple(288 + 6 * i for i in range(48)), tuple(range(24)))
# tiny66 (k = 46), E = 57 (odd): the first and last columns are not sent, a symbol runs across k and the
# punctured run 45..47, and shortened bit 44 sits in the last, partial ubits word
RM_T66_57 = RateMatch((0, 7, 45, 46, 47, 65), (1, 33, 44))
RM_T66_54 = RateMatch((0, 7, 10, 20, 45, 46, 47, 50, 65), (1, 33, 44))                        # bps 2 and 6
RM_T68_52 = RateMatch((0, 7, 10, 20, 45, 46, 47, 50, 51, 60, 61, 62, 67), (1, 33, 44))        # bps 4
# the n = 1440 IRA graph (k = 720): shortening changes the accumulated parities; E = 1248
RM_IRA = RateMatch(tuple(720 + 4 + 5 * i for i in range(144)), tuple(range(720 - 48, 720)))

_DECODERS = {}


def _decoder(name, frames):
    from ldpc_amd.device import Decoder, Graph
    if (name, frames) not in _DECODERS:
        _DECODERS[name, frames] = Decoder(Graph.cached(_graph_h(name)[0]), frames)
    return _DECODERS[name, frames]


@pytest.fixture(scope="module", autouse=True)
def _close_decoders():
    yield
    for dec in _DECODERS.values():
        dec.close()
    _DECODERS.clear()


@functools.lru_cache(maxsize=None)
def _bits(name, rm, snr_point, frame0, count):
    H, ira = _graph_h(name)
    u, c = ratematch_ref.bits(H, ira, rm, SEED, snr_point, frame0, count)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c


def test_patterns_are_what_the_cases_say():
    for name, rm, E in ((W576, RM_W576, 504), ("tiny66", RM_T66_57, 57), ("tiny66", RM_T66_54, 54),
                        ("tiny68", RM_T68_52, 52), ("ira1440", RM_IRA, 1248)):
        m, n = _graph_h(name)[0].shape
        rm.validate(n, n - m)
        assert rm.n_transmitted(n) == E and len(rm.transmitted(n)) == E
    assert 504 % 6 == 0 and 504 % 4 == 0 and 1248 % 6 == 0 and 1248 % 4 == 0 and 54 % 6 == 0 and 52 % 4 == 0
    tx = RM_T66_57.transmitted(66)
    assert tx[0] != 0 and tx[-1] != 65 and 44 in RM_T66_57.shortened and 46 // 32 == 44 // 32 == 1


# ------------------------------------------------------------ 1. generator
GEN_CASES = [(W576, RM_W576, s) for s in ALL_SPECS] + \
            [("tiny66", RM_T66_57, s) for s in ALL_SPECS if s.bps == 1] + \
            [("tiny66", RM_T66_54, s) for s in ALL_SPECS if s.bps in (2, 6)] + \
            [("tiny68", RM_T68_52, s) for s in ALL_SPECS if s.bps == 4] + \
            [("ira1440", RM_IRA, s) for s in ALL_SPECS]


@pytest.mark.parametrize("name,rm,spec", GEN_CASES, ids=[f"{n}-{_id(s)}" for n, _, s in GEN_CASES])
def test_generator_matches_restatement(gpu_available, name, rm, spec):
    """70 frames (a full tile and a ragged one) from frame 1000 of SNR point 3:
    u and the codeword signs identical, |llr - restatement| <= 1e-12 max(1, M) +
    1e-12 |llr| on the transmitted columns (test_gpu_channel.py's bound),
    punctured columns exactly +0.0, shortened columns exactly -1e4."""
    count, frame0, p = 70, 1000, 3
    sigma = GEN_SIGMA[spec.bps]
    dec = _decoder(name, 128)
    dec.set_channel(spec)
    dec.set_rate_match(rm)
    try:
        assert dec.rate_match == rm and dec.channel == spec
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
        _, quiet = dec.generate(SEED, p, 1e-6, frame0, count)
    finally:
        dec.set_rate_match(None)
        dec.set_channel(None)
    uo, co = _bits(name, rm, p, frame0, count)
    n = co.shape[1]
    tx, pu, sh = rm.transmitted(n), list(rm.punctured), list(rm.shortened)
    np.testing.assert_array_equal(u, uo)
    assert not u[:, sh].any()
    np.testing.assert_array_equal(quiet[:, tx] > 0, co[:, tx] == 1)
    want, M = ratematch_ref.frames_llr(spec, rm, co, SEED, p, sigma, frame0)
    for got in (llr, quiet):
        assert (got[:, pu] == 0.0).all() and not np.signbit(got[:, pu]).any(), "punctured columns are not +0.0"
        assert (got[:, sh] == -KNOWN_LLR).all(), "shortened columns are not -1e4"
    bound = 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want)
    ratio = float((np.abs(llr - want) / bound).max())
    print(f"{name} {_id(spec)} E={len(tx)}: max |delta| / bound = {ratio:.3g}, largest metric {M.max():.4g}")
    assert np.isfinite(llr).all()
    assert ratio <= 1.0, f"{name} {_id(spec)}: |delta| is {ratio:.3g} x the bound"


# ------------------------------- 2. all three output forms carry the same frames
MC_SPECS = [ChannelSpec("rayleigh", "bpsk", "exact"), ChannelSpec("awgn", "qam16", "maxlog")]
MC_EBN0 = (4.0, 8.0)  # inside the waterfall, then error-free (found on the CPU)
MC_B, MC_T = 200, 20
MC_Q_SCALE = 1.0


@functools.lru_cache(maxsize=None)
def _w576():
    edd = ldpc_amd.load_committed_code(W576)
    return edd, edd.physical_matrix()


def _mc_sigmas(spec):
    rate = RM_W576.effective_rate(576, 288)
    assert rate == 264 / 504
    return [sigma_for_ebn0(e, rate, spec.bps) for e in MC_EBN0]


@functools.lru_cache(maxsize=None)
def _mc_frames(spec):
    """The frames generate() returns under spec and the pattern at the two points (read-only)."""
    dec = _decoder(W576, 256)
    dec.set_channel(spec)
    dec.set_rate_match(RM_W576)
    try:
        out = [dec.generate(SEED, p, s, 0, MC_B) for p, s in enumerate(_mc_sigmas(spec))]
    finally:
        dec.set_rate_match(None)
        dec.set_channel(None)
    for u, llr in out:
        u.setflags(write=False)
        llr.setflags(write=False)
    return out


def _counters(u, o):
    return oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])[[0, 1, 2, 3, 4, 6]]


@functools.lru_cache(maxsize=None)
def _mc_want(spec, schedule, qbits=None):
    """Per point: (the restatement's result, its counters) on _mc_frames."""
    Hp = _w576()[1]
    out = []
    for u, llr in _mc_frames(spec):
        if qbits is None:
            o = minsum_ref.decode(Hp, llr, MC_T, "nms", schedule, ALPHA, BETA)
            # a float decoder never moves a bit it was told: every shortened bit decodes to 0
            assert not (o["z"][:, list(RM_W576.shortened)] ^ 1).any()
        else:
            o = qminsum_ref.decode(Hp, llr, MC_T, "nms", schedule, qbits, MC_Q_SCALE, 12)
        out.append((o, _counters(u, o)))
    print(f"{_id(spec)} {schedule} q={qbits}: restatement failures {out[0][1][1]} / {out[1][1][1]} of {MC_B}")
    assert 0 < out[0][1][1] < MC_B, (spec, schedule, qbits, out[0][1])
    assert out[1][1][1] == 0, (spec, schedule, qbits, out[1][1])
    return out


def _run(spec, **kw):
    from ldpc_amd.device import Graph
    dec = _decoder(W576, 256)
    gp = Graph.cached(_w576()[1])
    dec.set_channel(spec)
    dec.set_rate_match(RM_W576)
    try:
        return dec.phys_mc_run(gp, SEED, _mc_sigmas(spec), MC_B, 0, MC_T, cn="nms", alpha=ALPHA, **kw)
    finally:
        dec.set_rate_match(None)
        dec.set_channel(None)


MC_PATHS = [("flooding", {}), ("layered", {}), ("flooding", {"hbm": True}), ("layered", {"tile": True})]


@pytest.mark.parametrize("spec", MC_SPECS, ids=_id)
@pytest.mark.parametrize("schedule,flags", MC_PATHS, ids=["flooding-lds", "layered-lds", "flooding-hbm", "layered-tile"])
def test_monte_carlo_counters_equal_restatement(gpu_available, spec, schedule, flags):
    want = _mc_want(spec, schedule)
    got = _run(spec, schedule=schedule, **flags)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"{_id(spec)} {schedule} {flags} point {p}")


@pytest.mark.parametrize("spec", MC_SPECS, ids=_id)
@pytest.mark.parametrize("schedule", ["flooding", "layered"])
@pytest.mark.parametrize("qtile", [False, True], ids=["q6-lds", "q6-tile"])
def test_fixed_point_counters_equal_restatement(gpu_available, spec, schedule, qtile):
    """6-bit messages at one quantizer step per unit of LLR: the shortened
    columns' Lambda = +1e4 saturates to +Qmax."""
    want = _mc_want(spec, schedule, 6)
    got = _run(spec, schedule=schedule, qbits=6, llr_scale=MC_Q_SCALE, qtile=qtile)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w,
                                      err_msg=f"{_id(spec)} q6 {schedule} qtile={qtile} point {p}")


# ------------------------------------------- 3. simulate() and the failed frames
@pytest.mark.parametrize("spec", MC_SPECS, ids=_id)
def test_simulate_and_failed_frames(gpu_available, spec):
    """mc.simulate with rate_match on the Eb/N0 axis reproduces the counters
    (the axis took the effective rate), the BER counts k - n_short bits, and
    every failed-frame record regenerates, on that decoder, to a frame the
    restatement also fails, with the recorded info-bit errors."""
    from ldpc_amd.device import Graph
    want = _mc_want(spec, "layered")
    res, ctr, st = mc.simulate(W576, list(MC_EBN0), MC_B, MC_T, seed=SEED, mode="physical", cn_rule="nms",
                               schedule="layered", alpha=ALPHA, channel=spec, snr_axis="ebn0", stats=True,
                               max_failed=8, rate_match=RM_W576)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"simulate point {p}")
        assert res.snr_points[p].failed_blocks == int(w[1])
        assert res.snr_points[p].ber == int(w[2]) / (264 * MC_B)
    assert res.snr_points[0].ber > 0.0
    assert (res.config.n, res.config.m, res.config.k) == (576, 288, 288) and res.config.rate == 264 / 504
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    sig = _mc_sigmas(spec)
    dec.set_channel(spec)
    dec.set_rate_match(RM_W576)
    dec.mc_stats(True, 8)
    try:
        got = dec.phys_mc_run(gp, SEED, sig, MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA)
        np.testing.assert_array_equal(got[0][[0, 1, 2, 3, 4, 6]], want[0][1])
        rec = dec.mc_stats_read(0, MC_T)
        # which failures are kept is the workgroups' order of arrival: simulate()'s eight need not be these
        assert len(st[0]["failed"]) == len(rec["failed"]) and st[0]["hist"][MC_T] == int(want[0][1][1])
        assert len(rec["failed"]) == min(8, int(want[0][1][1])) and len(rec["failed"]) > 0
        for index, errs in rec["failed"]:
            u, llr = dec.generate(SEED, 0, sig[0], int(index), 1)
            np.testing.assert_array_equal(llr[0], _mc_frames(spec)[0][1][int(index)])
            np.testing.assert_array_equal(u[0], _mc_frames(spec)[0][0][int(index)])
            o = minsum_ref.decode(Hp, llr, MC_T, "nms", "layered", ALPHA, BETA)
            assert o["status"][0] != 0, f"frame {index} does not fail in the restatement"
            assert int(((o["z"][0, :u.shape[1]] ^ 1) != u[0]).sum()) == int(errs)
        assert dec.mc_stats_read(1, MC_T)["hist"][MC_T] == 0
    finally:
        dec.mc_stats(False)
        dec.set_rate_match(None)
        dec.set_channel(None)


# ------------------------------------------- 4. nothing moved, nothing stale
def test_no_pattern_is_untouched_and_nothing_stale_survives(gpu_available):
    """One decoder: no pattern, pattern A, cleared, pattern B (its columns
    disjoint from A's), cleared.  The three no-pattern passes give identical
    frames, counters and launch counts, equal to a decoder's that never saw a
    pattern and to the committed CPU frame source; B's frames equal the
    restatement, so no value of A survives in any of the three output forms."""
    from ldpc_amd.device import Decoder, Graph
    H = hstd_for(W576)
    edd, Hp = _w576()
    gp = Graph.cached(Hp)
    B, T = 96, 10
    spec = ChannelSpec("awgn", "qam16", "maxlog")
    ref_sig = [oracle.sigma_for_snr(s) for s in (-2.5, 2.0)]
    mod_sig = [sigma_for_ebn0(e, 0.5, spec.bps) for e in (3.0, 8.0)]
    A = RM_W576
    Bp = RateMatch(tuple(288 + 6 * i + 3 for i in range(48)), tuple(range(100, 124)))
    assert not (set(A.punctured) | set(A.shortened)) & (set(Bp.punctured) | set(Bp.shortened))

    def no_pattern_pass(dec):
        assert dec.rate_match == RateMatch() and dec.channel == ChannelSpec()
        out = list(dec.generate(SEED, 3, ref_sig[1], 1000, B))
        dec.profile(True)
        out.append(dec.phys_mc_run(gp, SEED, ref_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA))
        prof = dec.profile_read()
        out.append(dec.mc_run(SEED, ref_sig, B, 0, T, nllr=True, static=True))
        prof2 = dec.profile_read()
        dec.set_channel(spec)
        try:
            out.extend(dec.generate(SEED, 3, mod_sig[0], 1000, B))
            out.append(dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA))
            out.append(dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, tile=True))
            prof3 = dec.profile_read()
        finally:
            dec.set_channel(None)
            dec.profile(False)
        out.append(np.array([prof["generate"][1], prof2["generate"][1], prof3["generate"][1]]))
        return out

    def pattern_pass(dec, rm):
        """Every output form under the pattern; generate()'s frames against the restatement."""
        dec.set_channel(spec)
        dec.set_rate_match(rm)
        try:
            assert dec.rate_match == rm
            u, llr = dec.generate(SEED, 3, mod_sig[0], 1000, B)
            runs = [dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, **kw)
                    for kw in ({}, {"tile": True})]
            frames = [dec.generate(SEED, p, s, 0, B) for p, s in enumerate(mod_sig)]
        finally:
            dec.set_rate_match(RateMatch() if rm is Bp else None)  # an empty pattern is None
            dec.set_channel(None)
        uo, co = ratematch_ref.bits(H, False, rm, SEED, 3, 1000, B)
        want, M = ratematch_ref.frames_llr(spec, rm, co, SEED, 3, mod_sig[0], 1000)
        np.testing.assert_array_equal(u, uo)
        assert (np.abs(llr - want) <= 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want)).all()
        for p, (uf, lf) in enumerate(frames):
            o = minsum_ref.decode(Hp, lf, T, "nms", "layered", ALPHA, BETA)
            for r in runs:
                np.testing.assert_array_equal(r[p][[0, 1, 2, 3, 4, 6]], _counters(uf, o), err_msg=f"point {p}")

    fresh = Decoder(Graph.cached(H), B)
    dec = Decoder(Graph.cached(H), B)
    try:
        first = no_pattern_pass(dec)
        pattern_pass(dec, A)
        second = no_pattern_pass(dec)
        pattern_pass(dec, Bp)
        third = no_pattern_pass(dec)
        never = no_pattern_pass(fresh)
    finally:
        dec.close()
        fresh.close()
    for other in (second, third, never):
        assert len(other) == len(first)
        for a, b in zip(first, other):
            np.testing.assert_array_equal(a, b)  # bit for bit, launch counts included
    assert first[-1].tolist() == [len(ref_sig), len(ref_sig), 2 * len(mod_sig)]  # one generator stage per chunk
    uo, _, lo = oracle.generate_frames(H, SEED, 3, ref_sig[1], 1000, B)
    np.testing.assert_array_equal(first[0], uo)
    np.testing.assert_allclose(first[1], lo, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------ 5. refusals
def _einval(call, *needles):
    with pytest.raises(_lib.LdpcError) as e:
        call()
    assert e.value.code == _lib.LDPC_EINVAL, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def _raw_set(dec, punct, short, n_punct=None, n_short=None):
    """ldpc_rate_match_set itself (Decoder.set_rate_match validates before it calls)."""
    p, s = _lib.as_i32(punct), _lib.as_i32(short)
    return _lib.lib().ldpc_rate_match_set(
        dec._h, len(p) if n_punct is None else n_punct, _lib.i32p(p) if punct is not None and len(p) else None,
        len(s) if n_short is None else n_short, _lib.i32p(s) if short is not None and len(s) else None)


def test_refusals_leave_the_decoder_usable(gpu_available):
    from ldpc_amd.device import Graph
    L = _lib.lib()
    tiny = _decoder("tiny66", 128)  # n = 66, k = 46
    tiny.set_channel(ChannelSpec("awgn", "bpsk"))
    tiny.set_rate_match(RM_T66_57)
    try:
        bad = [("negative count", lambda: _raw_set(tiny, [], [], n_punct=-1), b"negative"),
               ("NULL list", lambda: _raw_set(tiny, [], [], n_short=2), b"NULL"),
               ("index n", lambda: _raw_set(tiny, [66], []), b"outside"),
               ("index -1", lambda: _raw_set(tiny, [3], [-1]), b"outside"),
               ("duplicate within", lambda: _raw_set(tiny, [5, 9, 5], []), b"twice"),
               ("duplicate across", lambda: _raw_set(tiny, [5], [5]), b"twice"),
               ("shortened >= k", lambda: _raw_set(tiny, [], [46]), b"information column"),
               ("E < 1", lambda: _raw_set(tiny, list(range(21, 66)), list(range(21))), b"E < 1"),
               ("k - n_short < 1", lambda: _raw_set(tiny, [], list(range(46))), b"information bit"),
               ("NULL decoder", lambda: L.ldpc_rate_match_set(None, 0, None, 0, None), b"NULL decoder")]
        for what, call, msg in bad:
            assert call() == _lib.LDPC_EINVAL, what
            assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
            assert tiny.rate_match == RM_T66_57, what  # the earlier pattern is in force
        for rm in (RateMatch((66,)), RateMatch((5,), (5,)), RateMatch((), (46,)), RateMatch((), tuple(range(46)))):
            with pytest.raises(ValueError):
                tiny.set_rate_match(rm)
        with pytest.raises(ValueError):
            tiny.set_rate_match("0:4")
        assert tiny.rate_match == RM_T66_57
        u, llr = tiny.generate(SEED, 3, 0.8, 1000, 70)  # usable, under the earlier pattern
        np.testing.assert_array_equal(u, _bits("tiny66", RM_T66_57, 3, 1000, 70)[0])
        assert (llr[:, list(RM_T66_57.punctured)] == 0.0).all()
        # E = 57 under QPSK
        tiny.set_channel(ChannelSpec("awgn", "qpsk"))
        _einval(lambda: tiny.generate(SEED, 0, 0.5, 0, 8), "E = 57", "bps = 2")
        _einval(lambda: tiny.phys_mc_run(Graph.cached(_graph_h("tiny66")[0]), SEED, [0.5], 8, 0, 5, cn="nms",
                                         schedule="layered", qbits=6), "E = 57", "bps = 2")
        # n = 66 does not divide by 4, E = 64 does: the pattern's check replaces the code length's
        tiny.set_channel(ChannelSpec("awgn", "qam16"))
        tiny.set_rate_match(RateMatch((0, 65)))
        assert np.isfinite(tiny.generate(SEED, 0, 0.3, 0, 8)[1]).all()
        tiny.set_rate_match(None)
        _einval(lambda: tiny.generate(SEED, 0, 0.3, 0, 8), "n = 66", "bps = 4")
    finally:
        tiny.set_rate_match(None)
        tiny.set_channel(None)
    # a pattern under the reference channel, in parity mode, with the test erasures
    dec = _decoder(W576, 128)
    gp = Graph.cached(_w576()[1])
    dec.set_rate_match(RM_W576)
    try:
        _einval(lambda: dec.generate(SEED, 0, 0.8, 0, 8), "reference channel")
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.8], 64, 0, 5), "reference channel")
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.8], 64, 0, 5, cn="nms", schedule="layered", qbits=6),
                "reference channel")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "physical mode")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5, static=True), "physical mode")
        _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "physical mode")
        dec.set_channel(ChannelSpec("awgn", "qam16"))
        _einval(lambda: dec.generate(SEED, 0, 0.3, 0, 8, test_zero=True), "LDPC_F_TEST_ZERO")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "physical mode")
        assert dec.rate_match == RM_W576
        u, _ = dec.generate(SEED, 3, GEN_SIGMA[4], 1000, 70)  # still usable under the pattern ...
        np.testing.assert_array_equal(u, _bits(W576, RM_W576, 3, 1000, 70)[0])
    finally:
        dec.set_rate_match(None)
        dec.set_channel(None)
    assert dec.mc_run(SEED, [0.8], 64, 0, 5)[0, 0] == 64  # ... and in parity mode after clearing it
    assert len(dec.frame_order(SEED, 0, 0.8, 0, 64)) == 64
