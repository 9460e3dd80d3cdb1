"""The physical-mode frame source under a bit interleaver
(ldpc_interleaver_set) and block fading (ldpc_fading_set) on the GPU.

1. generate() against the numpy restatement (tests/interleave_ref.py: the
   interleaved transmitted bits c[tx[pi]] through the whole constellation, block
   fades repeated, scattered back), on the smallest shapes at which each index
   computation can go wrong;
2. every output form and decoder sees the same frames: the Monte-Carlo counters
   of every decoder path equal the restatements' on the frames generate()
   returns;
3. mc.simulate with interleaver / fading_block, and the failed-frame records;
4. nothing moved, nothing stale: one decoder through set and cleared states;
5. the refusals.
"""
import functools

import numpy as np
import pytest

import bitflip_ref
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
from ldpc_amd.ratematch import KNOWN_LLR, RateMatch
from test_gpu_channel import ALL_SPECS, GEN_SIGMA, _graph_h, _id
from test_gpu_ratematch import RM_IRA, RM_T66_57, RM_T68_52, RM_W576

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
W576 = "wimax_576_0.5"
NONE = RateMatch()

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


def _set(dec, spec, rm, ilv, block_len):
    dec.set_channel(spec)
    dec.set_rate_match(rm)
    dec.set_interleaver(ilv)
    dec.set_fading_block(block_len)


def _clear(dec):
    dec.set_fading_block(1)
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


def _bound(want, M):
    """test_gpu_channel.py's bound: 1e-12 max(1, M) + 1e-12 |llr|."""
    return 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want)


@functools.lru_cache(maxsize=None)
def _ilv(kind, *args):
    return getattr(il, kind)(*args)


def test_interleavers_are_what_the_cases_say():
    assert il.regular_shape(576) == (24, 24) and il.regular_shape(52) == (4, 13)
    assert RM_W576.n_transmitted(576) == 504 and RM_T66_57.n_transmitted(66) == 57
    assert RM_T68_52.n_transmitted(68) == 52 and RM_IRA.n_transmitted(1440) == 1248
    assert il.s_distance_ok(_ilv("srandom", 1248, 12, 3).perm, 12)
    # block_len 5 on E = 504: the tile form's workgroups take 64 (BPSK, QPSK), 32 (16-QAM) and 21 (64-QAM)
    # units each, none a multiple of 5, so a fading block straddles two workgroups' ranges
    assert all(w % 5 for w in (64, 32, 21))
    # tiny66 under 64-QAM: 11 symbols in blocks of 3, the last block ragged.  BPSK in blocks of 3: positions 2 and
    # 3, the two of noise pair 1, lie in blocks 0 and 1.  E = 57 in blocks of 2: 29 blocks, the last of one bit
    assert 66 // 6 == 11 and 11 % 3 and 2 // 3 != 3 // 3 and 57 % 2 and -(-57 // 2) == 29


# ------------------------------------------------------------ 1. generator
def _bl(spec, block_len):
    return block_len if spec.model == "rayleigh" else 1


RAYLEIGH = [s for s in ALL_SPECS if s.model == "rayleigh"]
GEN_CASES = (
    # no pattern: the n_fill = 0 path
    [(W576, NONE, ("regular", 576), 1, s) for s in ALL_SPECS] +
    [(W576, RM_W576, ("random", 504, 7), _bl(s, 5), s) for s in ALL_SPECS] +
    [("tiny66", NONE, ("block", 66, 6), _bl(s, 3), s) for s in ALL_SPECS if s.bps in (1, 2, 6)] +
    [("tiny66", RM_T66_57, ("random", 57, 7), b, s) for s in RAYLEIGH if s.bps == 1 for b in (2, 64)] +
    [("tiny68", RM_T68_52, ("regular", 52), _bl(s, 4), s) for s in ALL_SPECS if s.bps == 4] +
    [("ira1440", RM_IRA, ("srandom", 1248, 12, 3), _bl(s, 40), s) for s in ALL_SPECS] +
    # block fading alone: the kernels without a table
    [(W576, NONE, None, b, s) for s in RAYLEIGH for b in (5, 10 ** 6)])


def _case_id(case):
    name, rm, ilv, bl, spec = case
    return f"{name}-{len(rm.punctured) + len(rm.shortened)}unsent-{'noil' if ilv is None else ilv[0]}-L{bl}-{_id(spec)}"


@pytest.mark.parametrize("case", GEN_CASES, ids=[_case_id(c) for c in GEN_CASES])
def test_generator_matches_restatement(gpu_available, case):
    """70 frames (a full tile and a ragged one) from frame 1000 of SNR point 3:
    u identical, the signs at sigma = 1e-6 are the codeword, punctured columns
    exactly +0.0, shortened columns exactly -1e4, |llr - restatement| <=
    1e-12 max(1, M) + 1e-12 |llr| (test_gpu_channel.py's bound)."""
    name, rm, ilv, block_len, spec = case
    ilv = None if ilv is None else _ilv(*ilv)
    perm = None if ilv is None else ilv.perm
    count, frame0, p = 70, 1000, 3
    sigma = GEN_SIGMA[spec.bps]
    dec = _decoder(name, 128)
    _set(dec, spec, rm, ilv, block_len)
    try:
        assert dec.rate_match == rm and dec.channel == spec and dec.fading_block == block_len
        assert (dec.interleaver is None) if ilv is None else (dec.interleaver.perm == perm)
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
        _, quiet = dec.generate(SEED, p, 1e-6, frame0, count)
    finally:
        _clear(dec)
    uo, co = _bits(name, rm, p, frame0, count)
    n = co.shape[1]
    tx, pu, sh = rm.transmitted(n), list(rm.punctured), list(rm.shortened)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_array_equal(quiet[:, tx] > 0, co[:, tx] == 1)
    want, M = interleave_ref.frames_llr(spec, rm, perm, block_len, co, SEED, p, sigma, frame0)
    for got in (llr, quiet):
        assert (got[:, pu] == 0.0).all() and not np.signbit(got[:, pu]).any(), "punctured columns are not +0.0"
        assert (got[:, sh] == -KNOWN_LLR).all(), "shortened columns are not -1e4"
    ratio = float((np.abs(llr - want) / _bound(want, M)).max())
    print(f"{_case_id(case)}: max |delta| / bound = {ratio:.3g}, largest metric {M.max():.4g}")
    assert np.isfinite(llr).all()
    assert ratio <= 1.0, f"{_case_id(case)}: |delta| is {ratio:.3g} x the bound"
    if ilv is not None and not ilv.is_identity:
        # the permutation is in force: the frames of no interleaver are further away than the bound
        plain, _ = interleave_ref.frames_llr(spec, rm, None, block_len, co, SEED, p, sigma, frame0)
        assert (np.abs(llr - plain) > _bound(plain, M)).any()


# ------------------- 2. every output form and decoder sees the same frames
# (spec, interleaver, block_len, the two Eb/N0 points, the fixed-point decoder's steps per unit of LLR).  The
# points were found on the CPU with the restatements: the first inside every message-passing decoder's waterfall
# (float: 13 / 12 of 200 fail under flooding / layered for Rayleigh, 27 / 16 for AWGN; q = 6: 58 / 53 and
# 161 / 149), the second error-free for all of them.  _mc_want asserts that.
MC_CASES = {
    ChannelSpec("rayleigh", "qam16", "exact"): (("regular", 576), 24, (10.0, 18.0), 0.125),
    ChannelSpec("awgn", "qam64", "maxlog"): (("random", 576, 7), 1, (7.0, 11.0), 0.5),
}
MC_SPECS = list(MC_CASES)
MC_B, MC_T = 200, 20


@functools.lru_cache(maxsize=None)
def _w576():
    edd = ldpc_amd.load_committed_code(W576)
    return edd, edd.physical_matrix()


def _mc_sigmas(spec):
    return [sigma_for_ebn0(e, 0.5, spec.bps) for e in MC_CASES[spec][2]]


def _mc_set(dec, spec):
    ilv, bl, _, _ = MC_CASES[spec]
    _set(dec, spec, None, _ilv(*ilv), bl)


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
            o = qminsum_ref.decode(Hp, llr, MC_T, "nms", schedule, qbits, MC_CASES[spec][3], 12)
        out.append((o, _counters(u, o)))
    print(f"{_id(spec)} {schedule} q={qbits}: restatement failures {out[0][1][1]} / {out[1][1][1]} of {MC_B}")
    assert 0 < out[0][1][1] < MC_B, (spec, schedule, qbits, out[0][1])
    assert out[1][1][1] == 0, (spec, schedule, qbits, out[1][1])
    return out


def test_monte_carlo_frames_are_the_restatements(gpu_available):
    """The frames the counters below are computed on are the interleaved, block-faded ones."""
    for spec in MC_SPECS:
        ilv, bl, _, _ = MC_CASES[spec]
        for p, (u, llr) in enumerate(_mc_frames(spec)):
            uo, co = _bits(W576, NONE, p, 0, MC_B)
            np.testing.assert_array_equal(u, uo)
            want, M = interleave_ref.frames_llr(spec, None, _ilv(*ilv).perm, bl, co, SEED, p, _mc_sigmas(spec)[p], 0)
            assert (np.abs(llr - want) <= _bound(want, M)).all(), (spec, p)


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
    got = _run(spec, schedule=schedule, qbits=6, llr_scale=MC_CASES[spec][3], qtile=qtile)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w,
                                      err_msg=f"{_id(spec)} q6 {schedule} qtile={qtile} point {p}")


@pytest.mark.parametrize("spec", MC_SPECS, ids=_id)
def test_bit_flipping_counters_equal_restatement(gpu_available, spec):
    """Hard-decision flipping (w = 0) on the same frames.  It is far from error-free at these points (59 and 197
    of 200 frames fail at the second ones on the CPU); what is checked is that it decodes the same frames."""
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


# ------------------------------------------- 3. simulate() and the failed frames
def test_simulate_and_failed_frames(gpu_available):
    """mc.simulate(interleaver="regular", fading_block=24) reproduces the
    counters, and every failed-frame record regenerates, on the decoder that
    recorded it, bit for bit to the frame generate() returned under the same
    settings -- a frame the restatement also fails, with the recorded errors."""
    from ldpc_amd.device import Graph
    spec = MC_SPECS[0]
    assert MC_CASES[spec][:2] == (("regular", 576), 24)
    want = _mc_want(spec, "layered")
    ebn0 = list(MC_CASES[spec][2])
    res, ctr, st = mc.simulate(W576, ebn0, MC_B, MC_T, seed=SEED, mode="physical", cn_rule="nms", schedule="layered",
                               alpha=ALPHA, channel=spec, snr_axis="ebn0", stats=True, max_failed=8,
                               interleaver="regular", fading_block=24)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"simulate point {p}")
        assert res.snr_points[p].failed_blocks == int(w[1])
    assert res.config.interleaver_type == "regular" and res.config.rate == 0.5
    # the same with the Interleaver itself
    _, ctr2 = mc.simulate(W576, ebn0, MC_B, MC_T, seed=SEED, mode="physical", cn_rule="nms", schedule="layered",
                          alpha=ALPHA, channel=spec, snr_axis="ebn0", interleaver=il.regular(576), fading_block=24)
    np.testing.assert_array_equal(ctr2, ctr)
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    sig = _mc_sigmas(spec)
    _mc_set(dec, spec)
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
        _clear(dec)


# ------------------------------------------- 4. nothing moved, nothing stale
def test_cleared_states_are_a_fresh_decoder(gpu_available):
    """One decoder: nothing set, interleaver A, cleared, block_len 7, cleared,
    a pattern with interleaver B, both cleared.  Every cleared state gives the
    frames and counters of a decoder that never saw a setting, bit for bit, under
    the reference channel and under a channel model; every set state gives the
    restatement's frames, so nothing of an earlier table survives."""
    from ldpc_amd.device import Decoder, Graph
    H = _graph_h(W576)[0]
    Hp = _w576()[1]
    gp = Graph.cached(Hp)
    B, T, p, frame0 = 96, 10, 3, 1000
    spec = ChannelSpec("rayleigh", "qam16", "maxlog")
    ref_sig = [oracle.sigma_for_snr(s) for s in (-2.5, 2.0)]
    mod_sig = [sigma_for_ebn0(e, 0.5, spec.bps) for e in (10.0, 18.0)]
    A, Bi = il.regular(576), il.random(504, 7)

    def cleared_pass(dec):
        assert dec.rate_match == NONE and dec.channel == ChannelSpec()
        assert dec.interleaver is None and dec.fading_block == 1
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

    def set_pass(dec, rm, ilv, block_len):
        """Every output form under the settings; generate()'s frames against the restatement."""
        _set(dec, spec, rm, ilv, block_len)
        try:
            u, llr = dec.generate(SEED, p, mod_sig[0], frame0, B)
            runs = [dec.phys_mc_run(gp, SEED, mod_sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, **kw)
                    for kw in ({}, {"tile": True})]
            frames = [dec.generate(SEED, q, s, 0, B) for q, s in enumerate(mod_sig)]
        finally:
            _clear(dec)
        rm = rm or NONE
        uo, co = _bits(W576, rm, p, frame0, B)
        want, M = interleave_ref.frames_llr(spec, rm, None if ilv is None else ilv.perm, block_len, co, SEED, p,
                                            mod_sig[0], frame0)
        np.testing.assert_array_equal(u, uo)
        assert (np.abs(llr - want) <= _bound(want, M)).all()
        for q, (uf, lf) in enumerate(frames):
            o = minsum_ref.decode(Hp, lf, T, "nms", "layered", ALPHA, BETA)
            for r in runs:
                np.testing.assert_array_equal(r[q][[0, 1, 2, 3, 4, 6]], _counters(uf, o), err_msg=f"point {q}")
        return llr

    fresh = Decoder(Graph.cached(H), B)
    dec = Decoder(Graph.cached(H), B)
    try:
        passes = [cleared_pass(dec)]
        with_a = set_pass(dec, None, A, 1)
        passes.append(cleared_pass(dec))
        with_7 = set_pass(dec, None, None, 7)
        passes.append(cleared_pass(dec))
        set_pass(dec, RM_W576, Bi, 7)
        passes.append(cleared_pass(dec))
        never = cleared_pass(fresh)
        # an identity interleaver: the table path with the columns in order gives the no-interleaver LLRs
        plain = passes[0][5]
        _set(dec, spec, None, il.identity(576), 1)
        try:
            ident = dec.generate(SEED, p, mod_sig[0], frame0, B)[1]
        finally:
            _clear(dec)
    finally:
        dec.close()
        fresh.close()
    for other in passes:
        assert len(other) == len(never)
        for a, b in zip(never, other):
            np.testing.assert_array_equal(a, b)  # bit for bit
    uo, co = _bits(W576, NONE, p, frame0, B)
    want, M = interleave_ref.frames_llr(spec, None, None, 1, co, SEED, p, mod_sig[0], frame0)
    assert (np.abs(plain - want) <= _bound(want, M)).all() and (np.abs(ident - want) <= _bound(want, M)).all()
    assert (np.abs(ident - plain) <= 2 * _bound(want, M)).all()
    # the set states did differ from the cleared one
    assert (np.abs(with_a - plain) > _bound(want, M)).any() and (np.abs(with_7 - plain) > _bound(want, M)).any()
    uo, _, lo = oracle.generate_frames(H, SEED, p, ref_sig[1], frame0, B)
    np.testing.assert_array_equal(never[0], uo)
    np.testing.assert_allclose(never[1], lo, rtol=1e-12, atol=1e-12)


# ------------------------------------------------------------ 5. refusals
def _einval(call, *needles):
    with pytest.raises(_lib.LdpcError) as e:
        call()
    assert e.value.code == _lib.LDPC_EINVAL, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def _raw_set(dec, perm, length=None):
    """ldpc_interleaver_set itself (the Interleaver class validates before Decoder.set_interleaver calls)."""
    a = _lib.as_i32(perm if perm is not None else [])
    return _lib.lib().ldpc_interleaver_set(dec._h, len(a) if length is None else length,
                                           _lib.i32p(a) if perm is not None and len(a) else None)


def test_refusals_leave_the_decoder_usable(gpu_available):
    import ctypes
    from ldpc_amd.device import Graph
    L = _lib.lib()
    tiny = _decoder("tiny66", 128)  # n = 66, k = 46
    spec = ChannelSpec("rayleigh", "bpsk")
    keep = il.random(57, 7)
    _set(tiny, spec, RM_T66_57, keep, 2)
    try:
        n32, buf = ctypes.c_int32(), np.zeros(57, np.int32)
        bad = [("negative length", lambda: _raw_set(tiny, None, -1), b"negative"),
               ("NULL perm", lambda: _raw_set(tiny, None, 3), b"NULL"),
               ("entry len", lambda: _raw_set(tiny, [0, 1, 3]), b"outside"),
               ("entry -1", lambda: _raw_set(tiny, [0, -1, 2]), b"outside"),
               ("duplicate", lambda: _raw_set(tiny, [0, 2, 2]), b"twice"),
               ("NULL decoder", lambda: L.ldpc_interleaver_set(None, 0, None), b"NULL decoder"),
               ("block_len 0", lambda: L.ldpc_fading_set(tiny._h, 0), b"block_len"),
               ("block_len -4", lambda: L.ldpc_fading_set(tiny._h, -4), b"block_len"),
               ("fading NULL decoder", lambda: L.ldpc_fading_set(None, 3), b"NULL decoder"),
               ("fading get NULL decoder", lambda: L.ldpc_fading_get(None, ctypes.byref(n32)), b"NULL decoder"),
               ("fading get NULL out", lambda: L.ldpc_fading_get(tiny._h, None), b"NULL"),
               ("get NULL decoder", lambda: L.ldpc_interleaver_get(None, ctypes.byref(n32), None, 0), b"NULL decoder"),
               ("get NULL len", lambda: L.ldpc_interleaver_get(tiny._h, None, None, 0), b"bad arguments"),
               ("get capacity", lambda: L.ldpc_interleaver_get(tiny._h, ctypes.byref(n32), _lib.i32p(buf), 56),
                b"too small"),
               ("get negative capacity", lambda: L.ldpc_interleaver_get(tiny._h, ctypes.byref(n32), _lib.i32p(buf), -1),
                b"bad arguments")]
        for what, call, msg in bad:
            assert call() == _lib.LDPC_EINVAL, what
            assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
            assert tiny.interleaver.perm == keep.perm and tiny.fading_block == 2, what  # the earlier settings hold
        assert not buf.any()
        for arg in ((0, 1, 2), "regular", 5):
            with pytest.raises(ValueError):
                tiny.set_interleaver(arg)
        for arg in (0, -1, 2.5, True, 2 ** 31):
            with pytest.raises((ValueError, _lib.LdpcError)):
                tiny.set_fading_block(arg)
        assert tiny.interleaver.perm == keep.perm and tiny.fading_block == 2
        u, llr = tiny.generate(SEED, 3, 0.8, 1000, 70)  # usable, under the earlier settings
        uo, co = _bits("tiny66", RM_T66_57, 3, 1000, 70)
        want, M = interleave_ref.frames_llr(spec, RM_T66_57, keep.perm, 2, co, SEED, 3, 0.8, 1000)
        np.testing.assert_array_equal(u, uo)
        assert (np.abs(llr - want) <= _bound(want, M)).all()
        # a length mismatch after the pattern changes: the interleaver stays 57 long, E becomes 66, then 64
        gt = Graph.cached(_graph_h("tiny66")[0])
        tiny.set_rate_match(None)
        _einval(lambda: tiny.generate(SEED, 0, 0.5, 0, 8), "ldpc_interleaver_set", "length 57", "E = 66", "clears")
        _einval(lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5), "length 57", "E = 66")
        _einval(lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5, cn="nms", schedule="layered"), "length 57")
        _einval(lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5, cn="nms", schedule="layered", qbits=6), "length 57")
        _einval(lambda: tiny.bitflip_mc_run(gt, SEED, [0.5], 8, 0, 5), "length 57", "E = 66")
        tiny.set_rate_match(RateMatch((0, 65)))
        _einval(lambda: tiny.generate(SEED, 0, 0.5, 0, 8), "length 57", "E = 64")
        tiny.set_rate_match(RM_T66_57)
        np.testing.assert_array_equal(tiny.generate(SEED, 3, 0.8, 1000, 70)[1], llr)  # the pattern back: as before
        # block fading needs the Rayleigh model
        tiny.set_channel(ChannelSpec("awgn", "bpsk"))
        _einval(lambda: tiny.generate(SEED, 0, 0.5, 0, 8), "ldpc_fading_set", "block_len = 2", "LDPC_CH_RAYLEIGH",
                "clears")
        _einval(lambda: tiny.phys_mc_run(gt, SEED, [0.5], 8, 0, 5), "block_len = 2")
        _einval(lambda: tiny.bitflip_mc_run(gt, SEED, [0.5], 8, 0, 5), "block_len = 2")
        tiny.set_fading_block(1)
        want, M = interleave_ref.frames_llr(ChannelSpec("awgn", "bpsk"), RM_T66_57, keep.perm, 1, co, SEED, 3, 0.8, 1000)
        assert (np.abs(tiny.generate(SEED, 3, 0.8, 1000, 70)[1] - want) <= _bound(want, M)).all()
    finally:
        _clear(tiny)
    # either setting under the reference channel and in parity mode
    dec = _decoder(W576, 128)
    gp = Graph.cached(_w576()[1])
    first = dec.generate(SEED, 3, 0.8, 1000, 70)
    dec.set_interleaver(il.regular(576))
    try:
        _einval(lambda: dec.generate(SEED, 0, 0.8, 0, 8), "ldpc_interleaver_set", "reference channel", "clears")
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.8], 64, 0, 5), "reference channel")
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.8], 64, 0, 5, cn="nms", schedule="layered", qbits=6),
                "reference channel")
        _einval(lambda: dec.bitflip_mc_run(gp, SEED, [0.8], 64, 0, 5), "reference channel")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "interleaver", "physical mode")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5, static=True), "interleaver")
        _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "interleaver")
        dec.set_channel(ChannelSpec("awgn", "qam16"))
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "physical mode")
        dec.set_channel(None)
        dec.set_interleaver(None)
        dec.set_fading_block(4)
        assert dec.fading_block == 4 and dec.channel == ChannelSpec()
        _einval(lambda: dec.generate(SEED, 0, 0.8, 0, 8), "ldpc_fading_set", "LDPC_CH_RAYLEIGH")
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.8], 64, 0, 5), "LDPC_CH_RAYLEIGH")
        _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "block fading", "ldpc_fading_set(d, 1)")
        _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "block fading")
        # the channel setter leaves the coherence length alone, and the other way round
        dec.set_channel(ChannelSpec("rayleigh", "qam16"))
        assert dec.fading_block == 4
        dec.set_fading_block(1)
        assert dec.channel == ChannelSpec("rayleigh", "qam16")
    finally:
        _clear(dec)
    again = dec.generate(SEED, 3, 0.8, 1000, 70)  # under the reference channel nothing changed
    np.testing.assert_array_equal(again[0], first[0])
    np.testing.assert_array_equal(again[1], first[1])
    assert dec.mc_run(SEED, [0.8], 64, 0, 5)[0, 0] == 64  # and parity mode runs after clearing
    assert len(dec.frame_order(SEED, 0, 0.8, 0, 64)) == 64
