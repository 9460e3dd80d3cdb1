"""The physical-mode frame source under a HARQ plan (ldpc_harq_set) on the GPU.

1. generate() against the numpy restatement (tests/harq_ref.py: every
   transmission through interleave_ref.sent_llr with its own Philox key,
   scattered and summed), on the smallest shapes at which each index computation
   can go wrong;
2. a one-transmission plan gives the numbers of the pattern + interleaver path;
3. every output form and decoder sees the same frames: the Monte-Carlo counters
   of every decoder path equal the restatements' on the frames generate()
   returns;
4. mc.simulate_harq against R separate runs, and the failed-frame records;
5. nothing moved, nothing stale: one decoder through set, changed and cleared
   plans; the refusals; ldpc_harq_get.
"""
import ctypes
import functools

import numpy as np
import pytest

import bitflip_ref
import harq_ref
import interleave_ref
import ldpc_amd
import minsum_ref
import oracle
import qminsum_ref
import ratematch_ref
from ldpc_amd import _lib
from ldpc_amd import interleave as il
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
from ldpc_amd.harq import HarqPlan
from ldpc_amd.ratematch import KNOWN_LLR, RateMatch
from test_gpu_channel import ALL_SPECS, GEN_SIGMA, _graph_h, _id
from test_gpu_ratematch import RM_IRA, RM_W576

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
W576 = "wimax_576_0.5"
NONE = RateMatch()
SHORT_IRA = RateMatch((), RM_IRA.shortened)

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


def _set(dec, spec, rm, plan, block_len):
    dec.set_channel(spec)
    dec.set_rate_match(rm)
    dec.set_harq(plan)
    dec.set_fading_block(block_len)


def _clear(dec):
    dec.set_fading_block(1)
    dec.set_harq(None)
    dec.set_interleaver(None)
    dec.set_rate_match(None)
    dec.set_channel(None)


@functools.lru_cache(maxsize=None)
def _bits(name, rm, snr_point, frame0, count):
    H, ira = _graph_h(name)
    u, c = ratematch_ref.bits(H, ira, rm, SEED, snr_point, frame0, count)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c


def _bl(spec, block_len):
    return block_len if spec.model == "rayleigh" else 1


# ------------------------------------------------------------ 1. generator
EXACT = [s for s in ALL_SPECS if s.demap == "exact"]
RAYLEIGH_EXACT = [s for s in EXACT if s.model == "rayleigh"]
_PERM576 = il.random(576, 7).perm
PLANS = {
    "chase3": HarqPlan.chase(576, 3),
    # offsets 0, 384, 192: columns sent once and twice, a wrap inside transmission 1
    "ir3x384": HarqPlan.ir(576, 3, 384),
    # unequal lengths in a permuted order: 36 columns of the second list repeat the first's, 36 are new, 36 never sent
    "uneven": HarqPlan.from_lists([_PERM576[:504], _PERM576[468:540]]),
    "t66-ir2x30": HarqPlan.ir(66, 2, 30),     # 64-QAM: 5 symbols each, columns 60 .. 65 never sent
    "t66-ir2x58": HarqPlan.ir(66, 2, 58),     # BPSK: 29 noise pairs, the second list wraps after 8 positions
    "t68-ir2x52": HarqPlan.ir(68, 2, 52),     # 16-QAM: 13 symbols, the second list wraps after 16 positions
    # IRA graph with shortened info columns: the buffer skips them, 1248 of its 1392 columns are sent once
    "ira-ir4x312": HarqPlan.ir(1440, 4, 312, shortened=RM_IRA.shortened),
}
GEN_CASES = (
    [(W576, NONE, "chase3", _bl(s, 5), s) for s in ALL_SPECS] +
    [(W576, NONE, "ir3x384", _bl(s, 5), s) for s in EXACT] +
    [(W576, NONE, "uneven", _bl(s, 5), s) for s in RAYLEIGH_EXACT] +
    [("tiny66", NONE, "t66-ir2x30", _bl(s, 3), s) for s in ALL_SPECS if s.bps == 6] +
    [("tiny66", NONE, "t66-ir2x58", b, s) for s in RAYLEIGH_EXACT if s.bps == 1 for b in (3, 64)] +
    [("tiny68", NONE, "t68-ir2x52", _bl(s, 4), s) for s in ALL_SPECS if s.bps == 4] +
    [("ira1440", SHORT_IRA, "ira-ir4x312", _bl(s, 40), s) for s in EXACT])


def _case_id(case):
    name, rm, plan, bl, spec = case
    return f"{name}-{plan}-L{bl}-{_id(spec)}"


def test_plans_are_what_the_cases_say():
    assert [t[0] for t in PLANS["ir3x384"].tx] == [0, 384, 192]
    assert (np.bincount(np.concatenate(PLANS["ir3x384"].truncated(2).tx), minlength=576)[[0, 191, 192, 575]]
            == [2, 2, 1, 1]).all()
    sent = np.bincount(np.concatenate(PLANS["uneven"].tx), minlength=576)
    assert PLANS["uneven"].lengths == (504, 72) and sorted(np.bincount(sent).tolist()) == [36, 36, 504]
    assert set(range(60, 66)).isdisjoint(np.concatenate(PLANS["t66-ir2x30"].tx))
    assert PLANS["t66-ir2x58"].tx[1][:9] == (58, 59, 60, 61, 62, 63, 64, 65, 0)
    # E = 58 in blocks of 3: 20 blocks, the last of one position; 64 >= 58: one fade per transmission
    assert -(-58 // 3) == 20 and 58 % 3 == 1
    ira = np.concatenate(PLANS["ira-ir4x312"].tx)
    assert len(set(ira)) == 1248 and set(ira).isdisjoint(RM_IRA.shortened) and ira.min() == 0


@pytest.mark.parametrize("case", GEN_CASES, ids=[_case_id(c) for c in GEN_CASES])
def test_generator_matches_restatement(gpu_available, case):
    """70 frames (a full tile and a ragged one) from frame 1000 of SNR point 3:
    u identical, the signs at sigma = 1e-6 are the codeword on every sent
    column, never-sent columns exactly +0.0, shortened columns exactly -1e4,
    |llr - restatement| <= the sum over the transmissions that carry the column
    of 1e-12 max(1, M_r) + 1e-12 |llr_r| (harq_ref.py); and the frames of the
    plan without its last transmission are further away than that."""
    name, rm, plan_name, block_len, spec = case
    plan = PLANS[plan_name]
    count, frame0, p = 70, 1000, 3
    sigma = GEN_SIGMA[spec.bps]
    dec = _decoder(name, 128)
    _set(dec, spec, rm, plan, block_len)
    try:
        assert dec.harq.tx == plan.tx and dec.rate_match == rm and dec.channel == spec
        assert dec.fading_block == block_len and dec.interleaver is None
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
        _, quiet = dec.generate(SEED, p, 1e-6, frame0, count)
        dec.set_harq(plan.truncated(plan.R - 1))
        _, shorter = dec.generate(SEED, p, sigma, frame0, count)
    finally:
        _clear(dec)
    uo, co = _bits(name, rm, p, frame0, count)
    n = co.shape[1]
    sent = sorted(set(c for t in plan.tx for c in t))
    sh = list(rm.shortened)
    never = sorted(set(range(n)) - set(sent) - set(sh))
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_array_equal(quiet[:, sent] > 0, co[:, sent] == 1)
    want, bound = harq_ref.frames_llr(spec, plan.tx, rm.shortened, block_len, co, SEED, p, sigma, frame0)
    for got in (llr, quiet, shorter):
        assert (got[:, never] == 0.0).all() and not np.signbit(got[:, never]).any(), "never-sent columns are not +0.0"
        assert (got[:, sh] == -KNOWN_LLR).all(), "shortened columns are not -1e4"
    assert np.isfinite(llr).all()
    ratio = float((np.abs(llr - want)[:, sent] / bound[:, sent]).max())
    print(f"{_case_id(case)}: max |delta| / bound = {ratio:.3g}")
    assert ratio <= 1.0, f"{_case_id(case)}: |delta| is {ratio:.3g} x the bound"
    # the last transmission is in force
    last = list(plan.tx[-1])
    assert (np.abs(llr - shorter)[:, last] > bound[:, last]).any()
    rest = sorted(set(range(n)) - set(last))
    np.testing.assert_array_equal(llr[:, rest], shorter[:, rest])


# ---------------------------------- 2. R = 1 is the old path's numbers
ONE_SPECS = [ChannelSpec("rayleigh", "bpsk"), ChannelSpec("awgn", "qpsk"), ChannelSpec("rayleigh", "qam16", "exact"),
             ChannelSpec("awgn", "qam64", "maxlog")]


@pytest.mark.parametrize("spec", ONE_SPECS, ids=_id)
def test_one_transmission_is_the_pattern_and_interleaver(gpu_available, spec):
    """The plan (tx[pi],) with the pattern's shortened columns against the
    pattern RM_W576 with the interleaver pi: u and llr equal as numbers."""
    ilv = il.random(504, 7)
    block_len = _bl(spec, 5)
    count, frame0, p = 70, 1000, 3
    dec = _decoder(W576, 128)
    try:
        dec.set_channel(spec)
        dec.set_fading_block(block_len)
        dec.set_rate_match(RM_W576)
        dec.set_interleaver(ilv)
        old = dec.generate(SEED, p, GEN_SIGMA[spec.bps], frame0, count)
        dec.set_interleaver(None)
        dec.set_rate_match(RateMatch((), RM_W576.shortened))
        dec.set_harq(HarqPlan.from_lists([interleave_ref.columns(RM_W576, ilv.perm, 576).tolist()]))
        new = dec.generate(SEED, p, GEN_SIGMA[spec.bps], frame0, count)
    finally:
        _clear(dec)
    assert (old[0] == new[0]).all() and (old[1] == new[1]).all()
    assert not np.signbit(new[1][:, list(RM_W576.punctured)]).any()
    assert (new[1][:, list(RM_W576.shortened)] == -KNOWN_LLR).all()


# ------------------- 3. every output form and decoder sees the same frames
# (spec, block_len, the two Eb/N0 points at rate 1/2, the fixed-point decoder's steps per unit of LLR) under
# MC_PLAN: 384 columns, then the other 192 and the first 192 again.  The points were found on the CPU with the
# restatements (harq_ref frames): the first inside every message-passing decoder's waterfall (float: 11 / 10 of
# 200 fail under flooding / layered for Rayleigh, 38 / 23 for AWGN; q = 6: 82 / 80 and 155 / 132; with the first
# transmission alone all 200 fail), the second error-free for all of them.  _mc_want asserts that of the frames
# generate() returns.
MC_PLAN = HarqPlan.ir(576, 2, 384)
MC_CASES = {
    ChannelSpec("rayleigh", "qam16", "exact"): (24, (8.0, 18.0), 0.125),
    ChannelSpec("awgn", "qam64", "maxlog"): (1, (6.0, 9.0), 0.5),
}
MC_SPECS = list(MC_CASES)
MC_B, MC_T = 200, 20


@functools.lru_cache(maxsize=None)
def _w576():
    edd = ldpc_amd.load_committed_code(W576)
    return edd, edd.physical_matrix()


def _mc_sigmas(spec):
    return [sigma_for_ebn0(e, 0.5, spec.bps) for e in MC_CASES[spec][1]]


def _mc_set(dec, spec, plan=MC_PLAN):
    _set(dec, spec, None, plan, MC_CASES[spec][0])


@functools.lru_cache(maxsize=None)
def _mc_frames(spec):
    """The frames generate() returns under the case's settings at the two points (read-only)."""
    dec = _decoder(W576, 256)
    _mc_set(dec, spec)
    try:
        out = [dec.generate(SEED, p, s, 0, MC_B) for p, s in enumerate(_mc_sigmas(spec))]
    finally:
        _clear(dec)
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
            o = qminsum_ref.decode(Hp, llr, MC_T, "nms", schedule, qbits, MC_CASES[spec][2], 12)
        out.append((o, _counters(u, o)))
    print(f"{_id(spec)} {schedule} q={qbits}: restatement failures {out[0][1][1]} / {out[1][1][1]} of {MC_B}")
    assert 0 < out[0][1][1] < MC_B, (spec, schedule, qbits, out[0][1])
    assert out[1][1][1] == 0, (spec, schedule, qbits, out[1][1])
    return out


def test_monte_carlo_frames_are_the_restatements(gpu_available):
    """The frames the counters below are computed on are the combined ones."""
    for spec in MC_SPECS:
        for p, (u, llr) in enumerate(_mc_frames(spec)):
            uo, co = _bits(W576, NONE, p, 0, MC_B)
            np.testing.assert_array_equal(u, uo)
            want, bound = harq_ref.frames_llr(spec, MC_PLAN.tx, (), MC_CASES[spec][0], co, SEED, p, _mc_sigmas(spec)[p], 0)
            assert (np.abs(llr - want) <= bound).all(), (spec, p)


def _run(spec, **kw):
    from ldpc_amd.device import Graph
    dec = _decoder(W576, 256)
    gp = Graph.cached(_w576()[1])
    _mc_set(dec, spec)
    try:
        return dec.phys_mc_run(gp, SEED, _mc_sigmas(spec), MC_B, 0, MC_T, cn="nms", alpha=ALPHA, **kw)
    finally:
        _clear(dec)


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
    want = _mc_want(spec, schedule, 6)
    got = _run(spec, schedule=schedule, qbits=6, llr_scale=MC_CASES[spec][2], qtile=qtile)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w,
                                      err_msg=f"{_id(spec)} q6 {schedule} qtile={qtile} point {p}")


@pytest.mark.parametrize("spec", MC_SPECS, ids=_id)
def test_bit_flipping_counters_equal_restatement(gpu_available, spec):
    """Hard-decision flipping (w = 0) on the same frames; what is checked is that it decodes the same frames."""
    from ldpc_amd.device import Graph
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    _mc_set(dec, spec)
    try:
        got = dec.bitflip_mc_run(gp, SEED, _mc_sigmas(spec), MC_B, 0, MC_T, weight=0.0)
    finally:
        _clear(dec)
    for p, (u, llr) in enumerate(_mc_frames(spec)):
        o = bitflip_ref.decode(Hp, llr, MC_T, 0.0, 0.0)
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], _counters(u, o), err_msg=f"{_id(spec)} point {p}")


# ------------------------------------------- 4. simulate_harq and the failed frames
def test_simulate_harq_and_failed_frames(gpu_available):
    """mc.simulate_harq's fer_after are the failed counts of R separate runs
    with the truncated plans, its other figures follow from the counters, and
    every failed-frame record of the last run regenerates, on a decoder with the
    same settings, bit for bit to the combined frame generate() returned."""
    from ldpc_amd.device import Graph
    spec = MC_SPECS[0]
    bl, ebn0, _ = MC_CASES[spec]
    # the axis is Eb/N0 at the first transmission's rate 288 / 384: the sigmas of the cases above are at rate 1/2
    ebn0_first = [e + 10.0 * np.log10(0.5 / 0.75) for e in ebn0]
    res = mc.simulate_harq(W576, ebn0_first, MC_B, MC_T, MC_PLAN, seed=SEED, cn_rule="nms", schedule="layered",
                           alpha=ALPHA, channel=spec, snr_axis="ebn0", fading_block=bl, stats=True, max_failed=8)
    sig = _mc_sigmas(spec)
    np.testing.assert_allclose(res["sigma"], sig, rtol=1e-12)
    sig = res["sigma"]
    assert res["plan"] == MC_PLAN.info() and res["counters"].shape == (2, 2, 7)
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    try:
        for r in (1, 2):
            _mc_set(dec, spec, MC_PLAN.truncated(r))
            dec.mc_stats(True, 8)
            got = dec.phys_mc_run(gp, SEED, sig, MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA)
            np.testing.assert_array_equal(res["counters"][r - 1], got)
            for p in range(2):
                assert res["points"][p]["fer_after"][r - 1] == got[p][1] / MC_B
        fails = res["counters"][:, :, 1]
        assert (fails[0] >= fails[1]).all() and fails[0, 0] > fails[1, 0] > 0, fails  # combining helps; some still fail
        for p, pt in enumerate(res["points"]):
            assert pt == {"snr_db": ebn0_first[p], "frames": MC_B,
                          **mc.harq_point(res["counters"][:, p], (384, 384), 288, 4)}
            assert pt["p_tx"] == [1.0, fails[0, p] / MC_B]
        # the records of the R = 2 run (dec still holds it)
        rec = dec.mc_stats_read(0, MC_T)
        assert len(res["stats"]) == 2 and res["stats"][1][0]["hist"][MC_T] == fails[1, 0] == rec["hist"][MC_T]
        assert len(rec["failed"]) == min(8, int(fails[1, 0])) > 0
        full = dec.generate(SEED, 0, sig[0], 0, MC_B)
        for index, errs in rec["failed"]:
            u, llr = dec.generate(SEED, 0, sig[0], int(index), 1)
            np.testing.assert_array_equal(llr[0], full[1][int(index)])
            np.testing.assert_array_equal(u[0], full[0][int(index)])
            o = minsum_ref.decode(Hp, llr, MC_T, "nms", "layered", ALPHA, BETA)
            assert o["status"][0] != 0, f"frame {index} does not fail in the restatement"
            assert int(((o["z"][0, :u.shape[1]] ^ 1) != u[0]).sum()) == int(errs)
    finally:
        dec.mc_stats(False)
        _clear(dec)


# ------------------------------------------- 5. nothing moved, nothing stale
def test_cleared_plans_are_a_fresh_decoder(gpu_available):
    """One decoder: nothing set, plan A, plan B (longer: the table grows), A
    again, cleared.  Cleared gives the frames and counters of a decoder that
    never saw a plan, bit for bit; every set state gives the restatement's
    frames, and a second run repeats the first."""
    from ldpc_amd.device import Decoder, Graph
    H = _graph_h(W576)[0]
    Hp = _w576()[1]
    gp = Graph.cached(Hp)
    B, T, p, frame0 = 96, 10, 3, 1000
    spec = ChannelSpec("rayleigh", "qam16", "maxlog")
    ref_sig = [oracle.sigma_for_snr(s) for s in (-2.5, 2.0)]
    mod_sig = [sigma_for_ebn0(e, 0.5, spec.bps) for e in (8.0, 16.0)]
    A, Bp = HarqPlan.chase(576, 2, 384), PLANS["ir3x384"]

    def cleared_pass(dec):
        assert dec.harq is None and dec.rate_match == NONE and dec.channel == ChannelSpec()
        out = list(dec.generate(SEED, p, ref_sig[1], frame0, B))
        out.append(dec.phys_mc_run(gp, SEED, ref_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA))
        out.append(dec.mc_run(SEED, ref_sig, B, 0, T, nllr=True, static=True))
        assert len(dec.frame_order(SEED, 0, ref_sig[0], 0, B)) == B
        dec.set_channel(spec)
        try:
            out.extend(dec.generate(SEED, p, mod_sig[0], frame0, B))
            out.append(dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA))
            out.append(dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, tile=True))
        finally:
            dec.set_channel(None)
        return out

    def set_pass(dec, plan, block_len):
        _set(dec, spec, None, plan, block_len)
        try:
            u, llr = dec.generate(SEED, p, mod_sig[0], frame0, B)
            runs = [dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, **kw)
                    for kw in ({}, {"tile": True}, {})]
            frames = [dec.generate(SEED, q, s, 0, B) for q, s in enumerate(mod_sig)]
            np.testing.assert_array_equal(dec.generate(SEED, p, mod_sig[0], frame0, B)[1], llr)  # a second run
        finally:
            _clear(dec)
        uo, co = _bits(W576, NONE, p, frame0, B)
        want, bound = harq_ref.frames_llr(spec, plan.tx, (), block_len, co, SEED, p, mod_sig[0], frame0)
        np.testing.assert_array_equal(u, uo)
        assert (np.abs(llr - want) <= bound).all()
        for q, (uf, lf) in enumerate(frames):
            o = minsum_ref.decode(Hp, lf, T, "nms", "layered", ALPHA, BETA)
            for r in runs:
                np.testing.assert_array_equal(r[q][[0, 1, 2, 3, 4, 6]], _counters(uf, o), err_msg=f"point {q}")
        return llr

    fresh = Decoder(Graph.cached(H), B)
    dec = Decoder(Graph.cached(H), B)
    try:
        passes = [cleared_pass(dec)]
        with_a = set_pass(dec, A, 1)
        with_b = set_pass(dec, Bp, 7)
        np.testing.assert_array_equal(set_pass(dec, A, 1), with_a)
        passes.append(cleared_pass(dec))
        never = cleared_pass(fresh)
    finally:
        dec.close()
        fresh.close()
    for other in passes:
        assert len(other) == len(never)
        for a, b in zip(never, other):
            np.testing.assert_array_equal(a, b)  # bit for bit
    assert not np.array_equal(with_a, with_b) and not np.array_equal(with_a[:, :384], never[5][:, :384])
    assert (with_a[:, 384:] == 0.0).all()


def _einval(call, *needles):
    with pytest.raises(_lib.LdpcError) as e:
        call()
    assert e.value.code == _lib.LDPC_EINVAL, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def _raw_set(dec, lens, cols, n_tx=None):
    """ldpc_harq_set itself (the HarqPlan class validates before Decoder.set_harq calls)."""
    a, c = _lib.as_i32(lens if lens is not None else []), _lib.as_i32(cols if cols is not None else [])
    return _lib.lib().ldpc_harq_set(dec._h, len(a) if n_tx is None else n_tx, _lib.i32p(a) if lens is not None else None,
                                    _lib.i32p(c) if cols is not None else None)


def test_refusals_leave_the_decoder_usable(gpu_available):
    from ldpc_amd.device import Graph
    L = _lib.lib()
    tiny = _decoder("tiny66", 128)  # n = 66, k = 46
    spec = ChannelSpec("rayleigh", "qpsk")
    keep = PLANS["t66-ir2x58"]
    _set(tiny, spec, None, keep, 3)
    try:
        n32, lens, buf = ctypes.c_int32(), np.zeros(8, np.int32), np.zeros(116, np.int32)
        bad = [("n_tx -1", lambda: _raw_set(tiny, None, None, -1), b"n_tx"),
               ("n_tx 9", lambda: _raw_set(tiny, [1] * 9, [0] * 9), b"LDPC_HARQ_MAX_TX"),
               ("NULL lists", lambda: _raw_set(tiny, None, None, 2), b"NULL"),
               ("NULL cols", lambda: _raw_set(tiny, [2], None), b"NULL"),
               ("tx_len 0", lambda: _raw_set(tiny, [2, 0], [0, 1]), b"< 1"),
               ("column n", lambda: _raw_set(tiny, [2], [0, 66]), b"outside"),
               ("column -1", lambda: _raw_set(tiny, [2], [-1, 0]), b"outside"),
               ("duplicate", lambda: _raw_set(tiny, [2, 3], [0, 1, 4, 5, 4]), b"twice"),
               ("NULL decoder", lambda: L.ldpc_harq_set(None, 0, None, None), b"NULL decoder"),
               ("get NULL decoder", lambda: L.ldpc_harq_get(None, ctypes.byref(n32), None, None, 0), b"NULL decoder"),
               ("get NULL n_tx", lambda: L.ldpc_harq_get(tiny._h, None, None, None, 0), b"bad arguments"),
               ("get capacity", lambda: L.ldpc_harq_get(tiny._h, ctypes.byref(n32), _lib.i32p(lens), _lib.i32p(buf), 115),
                b"too small"),
               ("get negative capacity", lambda: L.ldpc_harq_get(tiny._h, ctypes.byref(n32), None, _lib.i32p(buf), -1),
                b"bad arguments")]
        for what, call, msg in bad:
            assert call() == _lib.LDPC_EINVAL, what
            assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
            assert tiny.harq.tx == keep.tx, what  # the earlier plan holds
        assert not buf.any()
        # ldpc_harq_get round-trips
        assert L.ldpc_harq_get(tiny._h, ctypes.byref(n32), _lib.i32p(lens), _lib.i32p(buf), 116) == 0
        assert n32.value == 2 and lens.tolist() == [58, 58, 0, 0, 0, 0, 0, 0]
        assert tuple(buf[:58]) == keep.tx[0] and tuple(buf[58:]) == keep.tx[1]
        for arg in (((0, 1),), "chase:2", 5):
            with pytest.raises(ValueError):
                tiny.set_harq(arg)
        with pytest.raises(ValueError, match="outside"):
            tiny.set_harq(HarqPlan(((0, 66),)))
        assert tiny.harq.tx == keep.tx
        u, llr = tiny.generate(SEED, 3, 0.6, 1000, 70)  # usable, under the earlier plan
        uo, co = _bits("tiny66", NONE, 3, 1000, 70)
        want, bound = harq_ref.frames_llr(spec, keep.tx, (), 3, co, SEED, 3, 0.6, 1000)
        np.testing.assert_array_equal(u, uo)
        assert (np.abs(llr - want) <= bound).all()
        gt = Graph.cached(_graph_h("tiny66")[0])
        every = [lambda: tiny.generate(SEED, 0, 0.5, 0, 8),
                 lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5),
                 lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5, cn="nms", schedule="layered"),
                 lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5, cn="nms", schedule="layered", qbits=6),
                 lambda: tiny.bitflip_mc_run(gt, SEED, [0.5], 8, 0, 5)]
        # E_r % bps: 58 is no multiple of 4; n % bps (66 % 4) is not what is checked
        tiny.set_channel(ChannelSpec("rayleigh", "qam16"))
        for call in every:
            _einval(call, "ldpc_harq_set", "E_r = 58", "bps = 4")
        tiny.set_harq(HarqPlan.ir(66, 2, 52))  # and 66 % 4 != 0 does not matter under a plan
        assert tiny.generate(SEED, 0, 0.5, 0, 8)[1].shape == (8, 66)
        tiny.set_harq(keep)
        tiny.set_channel(spec)
        # an interleaver
        tiny.set_interleaver(il.random(66, 7))
        for call in every:
            _einval(call, "ldpc_harq_set", "ldpc_interleaver_set")
        tiny.set_interleaver(None)
        # a pattern with punctured columns, whether the plan sends them or not
        tiny.set_rate_match(RateMatch((64, 65), ()))
        for call in every:
            _einval(call, "ldpc_harq_set", "ldpc_rate_match_set", "punctures 2")
        # a plan column that the pattern shortens
        tiny.set_rate_match(RateMatch((), (7,)))
        for call in every:
            _einval(call, "ldpc_harq_set", "column 7", "shortens")
        tiny.set_rate_match(None)
        # test erasures
        _einval(lambda: tiny.generate(SEED, 0, 0.5, 0, 8, test_zero=True), "LDPC_F_TEST_ZERO", "ldpc_harq_set")
        # the reference channel, and parity mode
        tiny.set_channel(None)
        tiny.set_fading_block(1)
        for call in every:
            _einval(call, "ldpc_harq_set", "reference channel", "clears")
        assert tiny.harq.tx == keep.tx
        tiny.set_channel(spec)
        tiny.set_fading_block(3)
        np.testing.assert_array_equal(tiny.generate(SEED, 3, 0.6, 1000, 70)[1], llr)  # everything back: as before
    finally:
        _clear(tiny)
    dec = _decoder(W576, 128)
    first = dec.generate(SEED, 3, 0.8, 1000, 70)
    dec.set_harq(HarqPlan.chase(576, 2))
    try:
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "HARQ", "physical mode", "clears")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5, static=True), "HARQ")
        _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "HARQ")
    finally:
        _clear(dec)
    again = dec.generate(SEED, 3, 0.8, 1000, 70)  # under the reference channel nothing changed
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])
    assert dec.mc_run(SEED, [0.8], 64, 0, 5)[0, 0] == 64  # and parity mode runs after clearing
    assert len(dec.frame_order(SEED, 0, 0.8, 0, 64)) == 64
