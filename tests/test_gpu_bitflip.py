"""Physical mode's bit-flipping decoders on the GPU (include/ldpc_hip.h
"bit-flipping decoders"; csrc/phys_bitflip.hip).  The arithmetic is integer
counting plus at most one fp32 multiply and add, the library is built without
FMA contraction, so every output of both kernels must EQUAL the numpy
restatement (tests/bitflip_ref.py): z, conv, status, iters and synw."""
import ctypes
import functools

import numpy as np
import pytest

import bitflip_ref
import ldpc_amd
import mc_stats_ref
import oracle
import synth_graphs
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
from ldpc_amd.ratematch import RateMatch

pytestmark = pytest.mark.gpu

SEED = 20260213
KEYS = ("z", "conv", "status", "iters", "synw")
SLICED, GENERIC = "bitflip_sliced_kernel", "bitflip_kernel"


@functools.lru_cache(maxsize=None)
def _code(name):
    edd = ldpc_amd.load_committed_code(name)
    return edd, edd.physical_matrix()


@functools.lru_cache(maxsize=None)
def _frames(name, snr, count):
    edd, _ = _code(name)
    u, c, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(snr), 0, count)
    u.setflags(write=False)
    llr.setflags(write=False)
    return u, llr


def _frozen(r):
    for v in r.values():
        v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _ref(name, snr, count, T, w, theta, first=None):
    """The restatement's result on a committed code, computed once and shared (read-only)."""
    llr = _frames(name, snr, count)[1]
    return _frozen(bitflip_ref.decode(_code(name)[1], llr if first is None else llr[:first], T, w, theta))


@functools.lru_cache(maxsize=None)
def _synth_frames(name, sigma):
    H = synth_graphs.graph(name)
    llr = synth_graphs.noisy_frames(H.shape[1], sigma, 70, 1234)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _synth_ref(name, sigma, w, theta):
    return _frozen(bitflip_ref.decode(synth_graphs.graph(name), _synth_frames(name, sigma), 10, w, theta))


def _graph(H):
    from ldpc_amd.device import Graph
    return Graph.cached(H)


def _converged(r):
    return int((r["status"] == 0).sum())


def _assert_equal(got, want, what):
    for key in KEYS:
        assert got[key].dtype == want[key].dtype, f"{what}: {key} dtype"
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")


def _check_both_kernels(g, llr, T, w, theta, want, what):
    """Every kernel that takes (w, theta) against the restatement; with w == 0
    that is the sliced and the per-frame kernel, which then agree bit for bit."""
    from ldpc_amd.device import bitflip_decode, bitflip_kernel_name
    assert bitflip_kernel_name(g, w, generic=True) == GENERIC
    assert bitflip_kernel_name(g, w) == (SLICED if w == 0 else GENERIC)
    _assert_equal(bitflip_decode(g, llr, T, w, theta, generic=True), want, f"{what} generic")
    if w == 0:
        _assert_equal(bitflip_decode(g, llr, T, w, theta), want, f"{what} sliced")


COMMITTED = [("wimax_576_0.5", 0.0, 96, 20, 0.0, 0.0), ("wimax_576_0.5", 0.0, 96, 20, 0.5, 0.0),
             ("wimax_576_0.5", 0.0, 96, 20, 0.0, -1.0), ("wimax_2304_0.5", 0.5, 96, 20, 0.0, 0.0),
             ("wimax_2304_0.5", 0.5, 96, 20, 0.5, 0.0), ("wimax_2304_0.75A", 1.0, 96, 20, 0.0, 0.0)]


@pytest.mark.parametrize("name,snr,count,T,w,theta", COMMITTED)
def test_committed_codes_equal_restatement(gpu_available, name, snr, count, T, w, theta):
    want = _ref(name, snr, count, T, w, theta)
    print(f"{name} {snr} dB ({w}, {theta}): restatement converged {_converged(want)} of {count}")
    assert 3 <= _converged(want) <= count - 3  # both exits are exercised
    _check_both_kernels(_graph(_code(name)[1]), _frames(name, snr, count)[1], T, w, theta, want, name)


def test_bch_strip_undetected_errors(gpu_available):
    """Majority flipping converges to wrong codewords on this code: z of a
    converged frame is then not what was sent, and must still equal the restatement's."""
    name, snr, B, T = "BCH_7_4_1_strip", 0.0, 256, 10
    u, llr = _frames(name, snr, B)
    want = _ref(name, snr, B, T, 0.0, 0.0)
    ok = want["status"] == 0
    wrong = ((want["z"][:, :u.shape[1]] ^ 1) != u).any(axis=1)
    print(f"{name}: converged {int(ok.sum())} of {B}, to another codeword {int((ok & wrong).sum())}")
    assert (ok & wrong).sum() >= 3
    _check_both_kernels(_graph(_code(name)[1]), llr, T, 0.0, 0.0, want, name)


SYNTH = [(name, sigma, w, theta) for name, sigma in (("ragged", 0.5), ("widecol", 0.5), ("large", 0.45))
         for w, theta in ((0.0, 0.0), (0.25, 0.0), (0.0, -1.0))]


@pytest.mark.parametrize("name,sigma,w,theta", SYNTH)
def test_synthetic_graphs_equal_restatement(gpu_available, name, sigma, w, theta):
    """ragged: column degrees 0, 1, 2 and 8, n = 101; widecol: a column of 12 (a
    fourth counter plane); large: n = 2602, eleven columns per thread."""
    want = _synth_ref(name, sigma, w, theta)
    print(f"{name} ({w}, {theta}): restatement converged {_converged(want)} of 70")
    assert 3 <= _converged(want) <= 67
    _check_both_kernels(_graph(synth_graphs.graph(name)), _synth_frames(name, sigma), 10, w, theta, want, name)


def test_positive_theta_flips_empty_columns(gpu_available):
    """theta = +0.5: a column of degree 0 has Delta = 0 < theta and flips while its frame runs."""
    H = synth_graphs.graph("ragged")
    assert (synth_graphs.degrees(H)[1] == 0).any()
    want = _synth_ref("ragged", 0.5, 0.0, 0.5)
    _check_both_kernels(_graph(H), _synth_frames("ragged", 0.5), 10, 0.0, 0.5, want, "ragged theta 0.5")


@functools.lru_cache(maxsize=None)
def _deep_column_graph():
    """widecol's shape with a column of 40: six counter planes in the sliced kernel."""
    m, n = 61, 121
    degs = synth_graphs._cycle(m, (3, 4, 5, 6))
    return synth_graphs._deal(m, n, degs, synth_graphs.SEED + 40,
                              placed={n - 1: synth_graphs._rows_with(degs, synth_graphs.SEED + 41, 40, 3)})


@pytest.mark.parametrize("theta", [0.0, -1.0])
def test_column_of_forty(gpu_available, theta):
    H = _deep_column_graph()
    assert synth_graphs.degrees(H)[1].max() == 40
    llr = synth_graphs.noisy_frames(H.shape[1], 0.5, 70, 1234)
    want = bitflip_ref.decode(H, llr, 10, 0.0, theta)
    print(f"column of 40, theta {theta}: restatement converged {_converged(want)} of 70")
    _check_both_kernels(_graph(H), llr, 10, 0.0, theta, want, "column of 40")


def test_wide_columns_fall_back_to_the_per_frame_kernel(gpu_available):
    """H_std of wimax_576_0.5 has columns of up to 191 rows: no sliced kernel."""
    from ldpc_amd.device import bitflip_decode, bitflip_kernel_name
    name = "wimax_576_0.5"
    H = _code(name)[0]._h_std
    assert np.bincount(H.tocsr().indices).max() > 63
    g, llr = _graph(H), _frames(name, 0.0, 96)[1][:8]
    assert bitflip_kernel_name(g) == GENERIC
    _assert_equal(bitflip_decode(g, llr, 5), bitflip_ref.decode(H, llr, 5), "H_std")


@pytest.mark.parametrize("generic", [False, True], ids=["sliced", "generic"])
def test_edges_one_frame_one_iteration_ragged_tile(gpu_available, generic):
    from ldpc_amd.device import bitflip_decode
    name, snr = "wimax_576_0.5", 0.0
    g, llr = _graph(_code(name)[1]), _frames(name, snr, 130)[1]
    _assert_equal(bitflip_decode(g, llr[:1], 20, generic=generic), _ref(name, snr, 130, 20, 0.0, 0.0, first=1),
                  "one frame")
    _assert_equal(bitflip_decode(g, llr[:96], 1, generic=generic), _ref(name, snr, 130, 1, 0.0, 0.0, first=96), "T=1")
    # two full tiles and one of 2 frames
    _assert_equal(bitflip_decode(g, llr, 20, generic=generic), _ref(name, snr, 130, 20, 0.0, 0.0), "130 frames")


@pytest.mark.parametrize("generic", [False, True], ids=["sliced", "generic"])
def test_device_pointers_equal_host_path(gpu_available, generic):
    """LDPC_F_DEVICE_PTRS: buffers from the HIP runtime, the launch asynchronous on the caller's stream."""
    from test_gpu_device_ptrs import DevBuf, Hip
    hip = Hip()
    name, snr, B, T = "wimax_576_0.5", 0.0, 96, 20
    g, llr = _graph(_code(name)[1]), _frames(name, snr, B)[1]
    n = g.n
    out = {"z": DevBuf(hip, (B, n), np.uint8)}
    out.update({k: DevBuf(hip, (B,), np.int32, fill=-7) for k in KEYS[1:]})
    llr_d = DevBuf.of(hip, llr)
    flags = _lib.LDPC_F_DEVICE_PTRS | (_lib.LDPC_F_BF_GENERIC if generic else 0)
    s = ctypes.c_void_p()
    hip.ok(hip.rt.hipStreamCreate(ctypes.byref(s)), "hipStreamCreate")
    try:
        _lib.check("ldpc_bf_decode", _lib.gpu().ldpc_bf_decode(
            g.handle, B, llr_d.data_ptr(), T, flags, 0.0, 0.0, *(out[k].data_ptr() for k in KEYS), s.value))
        hip.ok(hip.rt.hipStreamSynchronize(s), "hipStreamSynchronize")
    finally:
        hip.rt.hipStreamDestroy(s)
    _assert_equal({k: out[k].numpy() for k in KEYS}, _ref(name, snr, B, T, 0.0, 0.0), "device pointers")
    # only conv asked for, null stream
    conv = DevBuf(hip, (B,), np.int32, fill=-7)
    _lib.check("ldpc_bf_decode", _lib.gpu().ldpc_bf_decode(
        g.handle, B, llr_d.data_ptr(), T, flags, 0.0, 0.0, None, conv.data_ptr(), None, None, None, None))
    hip.ok(hip.rt.hipDeviceSynchronize(), "hipDeviceSynchronize")
    np.testing.assert_array_equal(conv.numpy(), _ref(name, snr, B, T, 0.0, 0.0)["conv"])


# ------------------------------------------------------------ Monte-Carlo
MC_NAME, MC_B, MC_T = "wimax_576_0.5", 256, 20
MC_SNRS = (0.0, 1.0)
MC_RULES = [(0.0, 0.0, False), (0.0, 0.0, True), (0.5, 0.0, False)]


def _counters(u, o):
    w = oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])
    assert w[5] == 0
    return w


@pytest.fixture(scope="module")
def mc_dec(gpu_available):
    from ldpc_amd.device import Decoder
    dec = Decoder(_graph(_code(MC_NAME)[0]._h_std), MC_B)
    yield dec
    dec.close()


@pytest.fixture(scope="module")
def mc_frames(mc_dec):
    sig = [mc.sigma_for_snr(s) for s in MC_SNRS]
    return sig, [mc_dec.generate(SEED, p, sig[p], 0, MC_B) for p in range(len(sig))]


_MC_WANT = {}


def _mc_want(frames, w, theta, key="reference"):
    """The restatement's result per point on the frames generate() returned
    (`key` names the frame set), computed once and shared."""
    if (key, w, theta) not in _MC_WANT:
        _MC_WANT[key, w, theta] = [_frozen(bitflip_ref.decode(_code(MC_NAME)[1], llr, MC_T, w, theta))
                                   for _, llr in frames]
    return _MC_WANT[key, w, theta]


@pytest.mark.parametrize("w,theta,generic", MC_RULES, ids=["sliced", "generic", "gd"])
def test_monte_carlo_counters_equal_restatement(mc_dec, mc_frames, w, theta, generic):
    """The on-device Lambda is -(float)llr of the same fp64 value generate()
    returns, so all seven counters are EQUAL to the restatement's."""
    sig, frames = mc_frames
    gp = _graph(_code(MC_NAME)[1])
    got = mc_dec.bitflip_mc_run(gp, SEED, sig, MC_B, 0, MC_T, weight=w, theta=theta, generic=generic)
    want = _mc_want(frames, w, theta)
    for p, (u, _) in enumerate(frames):
        np.testing.assert_array_equal(got[p], _counters(u, want[p]), err_msg=f"point {p}")
    assert 3 <= _converged(want[0]) <= MC_B - 3


def test_monte_carlo_two_chunks_and_a_ragged_tile(mc_dec, mc_frames):
    """A decoder of 128 slots takes 200 frames as a chunk of 128 and one of 72 (a tile of 8)."""
    from ldpc_amd.device import Decoder
    sig, frames = mc_frames
    gp = _graph(_code(MC_NAME)[1])
    small = Decoder(_graph(_code(MC_NAME)[0]._h_std), 128)
    try:
        assert small.capacity == 128
        got = small.bitflip_mc_run(gp, SEED, sig[:1], 200, 0, MC_T)
    finally:
        small.close()
    u, llr = frames[0]
    o = {k: v[:200] for k, v in _mc_want(frames, 0.0, 0.0)[0].items()}
    np.testing.assert_array_equal(got[0], _counters(u[:200], o))


@pytest.mark.parametrize("w", [0.0, 0.5])
def test_monte_carlo_statistics_equal_restatement(mc_dec, mc_frames, w):
    sig, frames = mc_frames
    gp = _graph(_code(MC_NAME)[1])
    want = _mc_want(frames, w, 0.0)
    mc_dec.mc_stats(True, 64)
    try:
        got = mc_dec.bitflip_mc_run(gp, SEED, sig, MC_B, 0, MC_T, weight=w)
        stats = [mc_dec.mc_stats_read(p, MC_T) for p in range(len(sig))]
    finally:
        mc_dec.mc_stats(False)
    for p, (u, _) in enumerate(frames):
        np.testing.assert_array_equal(got[p], _counters(u, want[p]), err_msg=f"point {p}")
        ws = mc_stats_ref.stats(u, want[p], MC_T)
        ws["failed_dropped"] = max(0, len(ws["failed"]) - 64)
        ws["failed"] = ws["failed"][:64]
        if ws["failed_dropped"] == 0:
            mc_stats_ref.assert_equal(stats[p], ws, f"w={w} point {p}")
        else:  # which 64 of the failures are recorded is the device's order
            np.testing.assert_array_equal(stats[p]["hist"], ws["hist"])
            assert (stats[p]["undetected_frames"], stats[p]["undetected_bit_errors"]) == \
                (ws["undetected_frames"], ws["undetected_bit_errors"])
            assert stats[p]["failed_dropped"] == ws["failed_dropped"] and len(stats[p]["failed"]) == 64
            full = mc_stats_ref.stats(u, want[p], MC_T)["failed"]
            assert {tuple(r) for r in stats[p]["failed"]} <= {tuple(r) for r in full}
        mc_stats_ref.assert_identities(stats[p]["hist"], got[p])


# AWGN, 16-QAM, every sixth parity column punctured (--puncture k:n:6): E = 528.  With 48 columns unknown,
# plain flipping (w = 0) almost never converges (2 of 256 at 14 dB on the CPU); with the channel term
# (w = 0.5) the waterfall is at 8-11 dB Eb/N0: 97 of 256 converged at 9 dB on the CPU restatement's frames.
QAM_SPEC = ChannelSpec("awgn", "qam16", "exact")
QAM_RM = RateMatch(tuple(range(288, 576, 6)), ())
QAM_EBN0 = (9.0, 14.0)


def test_monte_carlo_qam16_punctured(mc_dec):
    gp = _graph(_code(MC_NAME)[1])
    rate = QAM_RM.effective_rate(576, 288)
    sig = [sigma_for_ebn0(e, rate, QAM_SPEC.bps) for e in QAM_EBN0]
    mc_dec.set_channel(QAM_SPEC)
    mc_dec.set_rate_match(QAM_RM)
    try:
        frames = [mc_dec.generate(SEED, p, s, 0, MC_B) for p, s in enumerate(sig)]
        got = {w: mc_dec.bitflip_mc_run(gp, SEED, sig, MC_B, 0, MC_T, weight=w) for w in (0.5, 0.0)}
    finally:
        mc_dec.set_rate_match(None)
        mc_dec.set_channel(None)
    for w in (0.5, 0.0):
        want = _mc_want(frames, w, 0.0, key="qam16")
        print(f"qam16 punctured w={w}: restatement converged {[_converged(o) for o in want]} of {MC_B}")
        for p, (u, llr) in enumerate(frames):
            assert (llr[:, list(QAM_RM.punctured)] == 0).all()
            np.testing.assert_array_equal(got[w][p], _counters(u, want[p]), err_msg=f"w={w} point {p}")
    assert 3 <= _converged(_mc_want(frames, 0.5, 0.0, key="qam16")[0]) <= MC_B - 3


def test_simulate(gpu_available, mc_frames):
    sig, frames = mc_frames
    for w in (0.0, 0.5):
        res, ctr = mc.simulate(MC_NAME, list(MC_SNRS), MC_B, MC_T, seed=SEED, mode="physical", decoder="bitflipping",
                               bf_weight=w)
        assert res.config.decoder_type == ("bitflipping" if w == 0 else "bitflipping-gd")
        want = _mc_want(frames, w, 0.0)
        for p, sp in enumerate(res.snr_points):
            c = _counters(frames[p][0], want[p])
            np.testing.assert_array_equal(ctr[p], c)
            assert (sp.total_blocks, sp.failed_blocks) == (MC_B, int(c[1]))


# ---------------------------------------------------------------- refusals
def test_refusals_through_the_raw_abi(gpu_available, mc_dec):
    L = _lib.gpu()
    name = "wimax_576_0.5"
    g = _graph(_code(name)[1])
    llr = np.ascontiguousarray(_frames(name, 0.0, 96)[1][:4])
    z = np.empty((4, g.n), np.uint8)
    nan, inf = float("nan"), float("inf")

    def decode(graph=g.handle, batch=4, p=_lib.ptr(llr), T=5, flags=0, w=0.0, th=0.0):
        return L.ldpc_bf_decode(graph, batch, p, T, flags, w, th, _lib.ptr(z), None, None, None, None, None)

    assert decode() == 0
    for kw in (dict(graph=None), dict(batch=0), dict(batch=-1), dict(p=None), dict(T=0), dict(w=-1.0), dict(w=nan),
               dict(w=inf), dict(th=nan), dict(th=inf), dict(flags=_lib.LDPC_F_PHYS_HBM), dict(flags=_lib.LDPC_F_NLLR),
               dict(flags=0x200)):
        assert decode(**kw) == _lib.LDPC_EINVAL, kw

    sig = (ctypes.c_double * 1)(0.8)
    out = (ctypes.c_int64 * 7)()

    def run(d=mc_dec._h, gp=g.handle, T=5, flags=0, w=0.0, th=0.0, counters=out):
        return L.ldpc_bf_mc_run(d, gp, SEED, 1, sig, 8, 0, T, flags, w, th, counters, None)

    assert run() == 0 and out[0] == 8
    for kw in (dict(d=None), dict(gp=None), dict(counters=None), dict(T=0), dict(w=-1.0), dict(w=nan), dict(th=inf),
               dict(flags=_lib.LDPC_F_DEVICE_PTRS), dict(flags=_lib.LDPC_F_PHYS_HBM)):
        assert run(**kw) == _lib.LDPC_EINVAL, kw
    assert L.ldpc_bf_kernel_name(g.handle, 0, -1.0) == b"" and L.ldpc_bf_lds_bytes(g.handle, 0, nan) == -1
    assert L.ldpc_bf_lds_bytes(g.handle, 0, 0.0) == 8 * (g.n + g.m)
    assert L.ldpc_bf_lds_bytes(g.handle, _lib.LDPC_F_BF_GENERIC, 0.0) == 4 * g.n + g.n + g.m


def test_dvbs2_profile_does_not_fit_lds(gpu_available):
    from ldpc_amd import ira
    from ldpc_amd.device import bitflip_decode, bitflip_kernel_name
    g = _graph(ira.dvbs2_profile_matrix())
    assert g.n == 64800
    for w in (0.0, 0.5):
        assert bitflip_kernel_name(g, w) == "" and bitflip_kernel_name(g, w, generic=True) == ""
        with pytest.raises(ldpc_amd.LdpcError) as e:
            bitflip_decode(g, np.zeros((1, g.n)), 5, w)
        assert e.value.code == _lib.LDPC_ERANGE and "HBM" in str(e.value)
