"""The physical-mode frame source under the channel models (ldpc_channel_set:
AWGN / Rayleigh, BPSK .. 64-QAM, exact / max-log) on the GPU.

1. generate() against the numpy restatement (tests/channel_ref.py: brute force
   over all 2^bps constellation points), for every spec, on wimax_576_0.5, on
   two tiny [A | I] graphs where a symbol straddles k and the symbol count is
   odd, and on an IRA graph;
2. the models are the right models: sign errors of the max-log LLRs per
   bit-position class against the closed-form error rate of nearest-point
   decisions (a wrong Gray table, a wrong d or a wrong sigma cannot pass);
3. the three output forms (fp64 tiles, fp32 rows, fp32 tiles) carry the same
   frames: the Monte-Carlo counters of every decoder path equal the
   restatements' on the frames generate() returns;
4. nothing moved: a decoder that never set a channel, and one that set one and
   went back, produce the frames and counters they always did;
5. the refusals.
"""
import functools

import numpy as np
import pytest
from scipy import sparse, stats

import channel_ref
import ldpc_amd
import minsum_ref
import oracle
import qminsum_ref
from conftest import hstd_for
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
W576 = "wimax_576_0.5"
MODS = ("bpsk", "qpsk", "qam16", "qam64")
ALL_SPECS = [ChannelSpec(model, mod, demap) for model in ("awgn", "rayleigh") for mod in MODS
             for demap in ("exact", "maxlog")]
# the generator test's noise per modulation: LLRs of a few units, every level decision in play
GEN_SIGMA = {1: 0.8, 2: 0.6, 4: 0.3, 6: 0.15}


def _id(spec):
    return f"{spec.model}-{spec.modulation}-{spec.demap}"


def tiny_graph(m, n, seed):
    """[A | I_m] with k = n - m information columns: every row has three A
    entries (so min-sum has a second minimum) and its identity column."""
    k = n - m
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(m):
        for c in sorted(rng.choice(k, 3, replace=False)):
            rows.append(r)
            cols.append(int(c))
        rows.append(r)
        cols.append(k + r)
    return sparse.csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, n))


@functools.lru_cache(maxsize=None)
def _graph_h(name):
    """(H the frame source encodes with, ira)."""
    if name == "tiny66":
        return tiny_graph(20, 66, 66), False
    if name == "tiny68":
        return tiny_graph(22, 68, 68), False
    if name == "ira1440":
        from ldpc_amd import ira
        return sparse.csr_matrix(ira.small_ira_matrix()), True
    return hstd_for(name), False


_DECODERS = {}


def _decoder(name, frames):
    """One decoder per graph and size for the whole module (closed by _close_decoders)."""
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
def _bits(name, snr_point, frame0, count):
    """(u, codeword) of the frames, from the committed CPU frame source (the bits do not depend on sigma)."""
    H, ira = _graph_h(name)
    u, c, _ = oracle.generate_frames(H, SEED, snr_point, 1.0, frame0, count, ira=ira)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c


@functools.lru_cache(maxsize=None)
def _ref(name, spec, snr_point, sigma, frame0, count):
    llr, M = channel_ref.frames_llr(spec, _bits(name, snr_point, frame0, count)[1], SEED, snr_point, sigma, frame0)
    llr.setflags(write=False)
    return llr, M


# ------------------------------------------------------------ 1. generator
GEN_CASES = [(W576, s) for s in ALL_SPECS] + \
            [("tiny66", s) for s in ALL_SPECS if s.bps in (1, 2, 6)] + \
            [("tiny68", s) for s in ALL_SPECS if s.bps == 4] + \
            [("ira1440", s) for s in ALL_SPECS]


@pytest.mark.parametrize("name,spec", GEN_CASES, ids=[f"{n}-{_id(s)}" for n, s in GEN_CASES])
def test_generator_matches_restatement(gpu_available, name, spec):
    """70 frames (a full tile and a ragged one) from frame 1000 of SNR point 3:
    u and the codeword identical, |llr - restatement| <= 1e-12 max(1, M) +
    1e-12 |llr| with M the frame's largest metric (the size of what cancels)."""
    count, frame0, p = 70, 1000, 3
    sigma = GEN_SIGMA[spec.bps]
    dec = _decoder(name, 128)
    dec.set_channel(spec)
    try:
        assert dec.channel == spec
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
        # noise far below d, and below h d for every fade drawn here (h < 1e-4 has probability 1e-8 a symbol):
        # the signs are the codeword
        _, quiet = dec.generate(SEED, p, 1e-6, frame0, count)
        if spec.bps <= 2:  # one bit per axis: one expression, whatever the demapper
            other = ChannelSpec(spec.model, spec.modulation, "maxlog" if spec.demap == "exact" else "exact")
            dec.set_channel(other)
            np.testing.assert_array_equal(dec.generate(SEED, p, sigma, frame0, count)[1], llr)
    finally:
        dec.set_channel(None)
    uo, co = _bits(name, p, frame0, count)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_array_equal(quiet > 0, co == 1)
    want, M = _ref(name, spec, p, sigma, frame0, count)
    bound = 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want)
    ratio = float((np.abs(llr - want) / bound).max())
    print(f"{name} {_id(spec)}: max |delta| / bound = {ratio:.3g}, largest metric {M.max():.4g}")
    assert np.isfinite(llr).all()
    assert ratio <= 1.0, f"{name} {_id(spec)}: |delta| is {ratio:.3g} x the bound"


# ------------------------------------------- 2. the models are the right models
# sigma per spec such that every bit-position class errs between 3 % and 20 %
# (channel_ref.expected_ber), found on the CPU
BER_SIGMA = {("awgn", "bpsk"): 0.845, ("awgn", "qpsk"): 0.6, ("awgn", "qam16"): 0.285, ("awgn", "qam64"): 0.16,
             ("rayleigh", "bpsk"): 0.585, ("rayleigh", "qpsk"): 0.415, ("rayleigh", "qam16"): 0.195,
             ("rayleigh", "qam64"): 0.11}


def _class_errors(spec, llr, c):
    cls = channel_ref.bit_classes(spec.bps, c.shape[1])
    wrong = (llr > 0) != (c == 1)
    ncls = int(cls.max()) + 1
    return np.array([int(wrong[:, cls == t].sum()) for t in range(ncls)]), \
        np.array([int((cls == t).sum()) * c.shape[0] for t in range(ncls)])


@pytest.mark.parametrize("model,mod", sorted(BER_SIGMA))
def test_sign_errors_match_closed_form(gpu_available, model, mod):
    """96 frames, max-log (its sign is the nearest-point decision): the errors
    of every bit-position class lie in the central 99.9 % binomial interval of
    the closed-form rate -- and so do the restatement's own."""
    spec = ChannelSpec(model, mod, "maxlog")
    sigma, count, p = BER_SIGMA[model, mod], 96, 1
    rate = channel_ref.expected_ber(spec, sigma)
    assert ((rate > 0.03) & (rate < 0.20)).all(), rate
    dec = _decoder(W576, 128)
    dec.set_channel(spec)
    try:
        _, llr = dec.generate(SEED, p, sigma, 0, count)
    finally:
        dec.set_channel(None)
    c = _bits(W576, p, 0, count)[1]
    got, total = _class_errors(spec, llr, c)
    ref, _ = _class_errors(spec, _ref(W576, spec, p, sigma, 0, count)[0], c)
    for t, (g, r, N, q) in enumerate(zip(got, ref, total, rate)):
        lo, hi = stats.binom.ppf(0.0005, N, q), stats.binom.ppf(0.9995, N, q)
        print(f"{model} {mod} a{t}: device {g}, restatement {r} of {N}; expected {q * N:.1f}, band [{lo:.0f}, {hi:.0f}]")
        assert lo <= r <= hi, f"restatement, class a{t}"
        assert lo <= g <= hi, f"device, class a{t}"


# ------------------------------- 3. all three output forms carry the same frames
# Eb/N0 (dB) per spec: a point inside the waterfall, then an error-free one (found on the CPU)
MC_CASES = {ChannelSpec("rayleigh", "qam16", "exact"): (6.0, 14.0),
            ChannelSpec("awgn", "qam64", "maxlog"): (6.5, 10.0)}
MC_B, MC_T = 200, 20
# the fixed-point cases' quantizer: a QAM demapper's LLRs reach tens to hundreds at these points, and
# with 4 steps per unit (the BPSK default) nearly all of them would sit at +-Qmax = 31
MC_Q_SCALE = 0.5


@functools.lru_cache(maxsize=None)
def _w576():
    edd = ldpc_amd.load_committed_code(W576)
    return edd, edd.physical_matrix()


def _mc_sigmas(spec):
    edd, _ = _w576()
    return [sigma_for_ebn0(e, edd._k / edd._n, spec.bps) for e in MC_CASES[spec]]


@functools.lru_cache(maxsize=None)
def _mc_frames(spec):
    """The frames generate() returns under spec at its two points (read-only), checked against the restatement."""
    dec = _decoder(W576, 256)
    dec.set_channel(spec)
    try:
        out = [dec.generate(SEED, p, s, 0, MC_B) for p, s in enumerate(_mc_sigmas(spec))]
    finally:
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
        else:
            o = qminsum_ref.decode(Hp, llr, MC_T, "nms", schedule, qbits, MC_Q_SCALE, 12)
        out.append((o, _counters(u, o)))
    # the first point is inside the waterfall, the second is error-free
    assert 0 < out[0][1][1] < MC_B, (spec, schedule, qbits, out[0][1])
    assert out[1][1][1] == 0, (spec, schedule, qbits, out[1][1])
    return out


MC_PATHS = [("flooding", {}), ("layered", {}), ("flooding", {"hbm": True}), ("layered", {"tile": True})]


@pytest.mark.parametrize("spec", list(MC_CASES), ids=_id)
@pytest.mark.parametrize("schedule,flags", MC_PATHS, ids=["flooding-lds", "layered-lds", "flooding-hbm", "layered-tile"])
def test_monte_carlo_counters_equal_restatement(gpu_available, spec, schedule, flags):
    from ldpc_amd.device import Graph
    dec = _decoder(W576, 256)
    gp = Graph.cached(_w576()[1])
    want = _mc_want(spec, schedule)
    dec.set_channel(spec)
    try:
        got = dec.phys_mc_run(gp, SEED, _mc_sigmas(spec), MC_B, 0, MC_T, cn="nms", schedule=schedule, alpha=ALPHA,
                              **flags)
    finally:
        dec.set_channel(None)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"{_id(spec)} {schedule} {flags} point {p}")


@pytest.mark.parametrize("spec", list(MC_CASES), ids=_id)
@pytest.mark.parametrize("qtile", [False, True], ids=["q6-lds", "q6-tile"])
def test_fixed_point_counters_equal_restatement(gpu_available, spec, qtile):
    from ldpc_amd.device import Graph
    dec = _decoder(W576, 256)
    gp = Graph.cached(_w576()[1])
    want = _mc_want(spec, "layered", 6)
    dec.set_channel(spec)
    try:
        got = dec.phys_mc_run(gp, SEED, _mc_sigmas(spec), MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA,
                              qbits=6, llr_scale=MC_Q_SCALE, qtile=qtile)
    finally:
        dec.set_channel(None)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"{_id(spec)} q6 qtile={qtile} point {p}")


@pytest.mark.parametrize("spec", list(MC_CASES), ids=_id)
def test_simulate_and_failed_frames(gpu_available, spec):
    """mc.simulate on the Eb/N0 axis reproduces the counters; every failed-frame
    record regenerates, on that decoder, to a frame the restatement also fails."""
    from ldpc_amd.device import Graph
    want = _mc_want(spec, "layered")
    res, ctr, st = mc.simulate(W576, list(MC_CASES[spec]), MC_B, MC_T, seed=SEED, mode="physical", cn_rule="nms",
                               schedule="layered", alpha=ALPHA, channel=spec, snr_axis="ebn0", stats=True,
                               max_failed=8)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"simulate point {p}")
        assert res.snr_points[p].failed_blocks == int(w[1])
    assert [sp.snr_db for sp in res.snr_points] == list(MC_CASES[spec])
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    sig = _mc_sigmas(spec)
    dec.set_channel(spec)
    dec.mc_stats(True, 8)
    try:
        got = dec.phys_mc_run(gp, SEED, sig, MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA)
        np.testing.assert_array_equal(got[0][[0, 1, 2, 3, 4, 6]], want[0][1])
        rec = dec.mc_stats_read(0, MC_T)
        assert len(rec["failed"]) == min(8, int(want[0][1][1])) and len(rec["failed"]) > 0
        for index, errs in rec["failed"]:
            u, llr = dec.generate(SEED, 0, sig[0], int(index), 1)
            np.testing.assert_array_equal(llr[0], _mc_frames(spec)[0][1][int(index)])
            o = minsum_ref.decode(Hp, llr, MC_T, "nms", "layered", ALPHA, BETA)
            assert o["status"][0] != 0, f"frame {index} does not fail in the restatement"
            assert int(((o["z"][0, :u.shape[1]] ^ 1) != u[0]).sum()) == int(errs)
        assert dec.mc_stats_read(1, MC_T)["hist"][MC_T] == 0
    finally:
        dec.mc_stats(False)
        dec.set_channel(None)


# ------------------------------------------------------------ 4. nothing moved
def test_reference_channel_is_untouched(gpu_available):
    """A decoder that never set a channel, and one that set a QAM channel and
    went back to the reference: generate(), phys_mc_run (NMS layered) and
    mc_run are what the committed CPU frame source and the restatements give,
    and the generator launches as often as before."""
    from ldpc_amd.device import Decoder, Graph
    H = hstd_for(W576)
    edd, Hp = _w576()
    gp = Graph.cached(Hp)
    B, T = 96, 10
    sig = [oracle.sigma_for_snr(s) for s in (-2.5, 2.0)]
    fresh = Decoder(Graph.cached(H), B)
    back = Decoder(Graph.cached(H), B)
    assert fresh.channel == ChannelSpec()
    back.set_channel(ChannelSpec("awgn", "qam64", "maxlog"))
    assert back.channel == ChannelSpec("awgn", "qam64", "maxlog")
    back.generate(SEED, 3, 0.2, 1000, B)  # the model's kernels ran on it
    back.set_channel(None)
    assert back.channel == ChannelSpec()
    seen = []
    for dec in (fresh, back):
        u, llr = dec.generate(SEED, 3, sig[1], 1000, B)
        uo, _, lo = oracle.generate_frames(H, SEED, 3, sig[1], 1000, B)
        np.testing.assert_array_equal(u, uo)
        np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
        dec.profile(True)
        phys = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA)
        prof_phys = dec.profile_read()
        par = dec.mc_run(SEED, sig, B, 0, T, nllr=True, static=True)
        prof_par = dec.profile_read()
        dec.profile(False)
        stream = dec.mc_run(SEED, sig, B, 0, T, nllr=True)
        k = edd._k
        for p, s in enumerate(sig):
            uf, lf = dec.generate(SEED, p, s, 0, B)
            up, _, lp = oracle.generate_frames(H, SEED, p, s, 0, B)
            np.testing.assert_array_equal(uf, up)
            np.testing.assert_allclose(lf, lp, rtol=1e-12, atol=1e-12)
            o = minsum_ref.decode(Hp, lf, T, "nms", "layered", ALPHA, BETA)
            np.testing.assert_array_equal(phys[p][[0, 1, 2, 3, 4, 6]], _counters(uf, o), err_msg=f"phys point {p}")
            o = oracle.spa_decode(H, lf, T, nllr=True)
            w = oracle.main_counters(uf, o["z"], o["status"], o["conv"],
                                     nllr_cnt=np.rint(o["nllr"] * k).astype(np.int64), iters=o["iters"])
            np.testing.assert_array_equal(par[p], w, err_msg=f"parity point {p}")
            np.testing.assert_array_equal(stream[p], w, err_msg=f"parity stream point {p}")
        seen.append((u, llr, phys, par, prof_phys["generate"][1], prof_par["generate"][1]))
    for a, b in zip(*seen):
        np.testing.assert_array_equal(a, b)  # bit for bit, launch counts included
    assert seen[0][4] == len(sig) and seen[0][5] == len(sig)  # one generator stage per chunk, as always


# ------------------------------------------------------------ 5. refusals
def _einval(call, *needles):
    with pytest.raises(_lib.LdpcError) as e:
        call()
    assert e.value.code == _lib.LDPC_EINVAL, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_refusals_leave_the_decoder_usable(gpu_available):
    from ldpc_amd.device import Decoder, Graph
    # BCH (n = 7) under QPSK
    H = hstd_for("BCH_7_4_1_strip")
    bch = Decoder(Graph.cached(H), 64)
    bch.set_channel(ChannelSpec("awgn", "qpsk"))
    _einval(lambda: bch.generate(SEED, 0, 0.5, 0, 8), "n = 7", "bps = 2")
    _einval(lambda: bch.phys_mc_run(Graph.cached(H), SEED, [0.5], 8, 0, 5), "n = 7", "bps = 2")
    bch.set_channel(ChannelSpec("awgn", "bpsk"))
    assert np.isfinite(bch.generate(SEED, 0, 0.5, 0, 8)[1]).all()
    bch.set_channel(None)
    u, llr = bch.generate(SEED, 0, 0.5, 0, 8)
    uo, _, lo = oracle.generate_frames(H, SEED, 0, 0.5, 0, 8)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
    # n = 66 under 16-QAM
    tiny = _decoder("tiny66", 128)
    tiny.set_channel(ChannelSpec("rayleigh", "qam16"))
    try:
        _einval(lambda: tiny.generate(SEED, 0, 0.3, 0, 8), "n = 66", "bps = 4")
        _einval(lambda: tiny.phys_mc_run(Graph.cached(_graph_h("tiny66")[0]), SEED, [0.3], 8, 0, 5, cn="nms",
                                         schedule="layered", qbits=6), "n = 66", "bps = 4")
    finally:
        tiny.set_channel(None)
    # parity mode and the test erasures belong to the reference channel
    dec = _decoder(W576, 128)
    dec.set_channel(ChannelSpec("awgn", "qam16"))
    try:
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "physical mode")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5, static=True), "physical mode")
        _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "physical mode")
        _einval(lambda: dec.generate(SEED, 0, 0.3, 0, 8, test_zero=True), "LDPC_F_TEST_ZERO", "reference channel")
        u, llr = dec.generate(SEED, 3, GEN_SIGMA[4], 1000, 70)  # still usable under the model ...
        np.testing.assert_array_equal(u, _bits(W576, 3, 1000, 70)[0])
    finally:
        dec.set_channel(None)
    assert dec.mc_run(SEED, [0.8], 64, 0, 5)[0, 0] == 64  # ... and in parity mode after going back
    assert len(dec.frame_order(SEED, 0, 0.8, 0, 64)) == 64
    # what set_channel itself refuses never reaches the library's state
    with pytest.raises(ValueError):
        dec.set_channel("awgn")
    assert dec.channel == ChannelSpec()
