"""The fixed-point min-sum decoder with the state in HBM (csrc/phys_qtile.hip:
phys_qlayer_tile_kernel, phys_qcn_tile_kernel): forced with qtile=True
(LDPC_F_QUANT_TILE) where the quantized state fits LDS, automatic on the
DVB-S2 profile (n = 64800), whose int8 / int16 state does not fit.

The contract is all-integer after the load, so every comparison is EQUALITY
with the numpy int32 restatement (tests/qminsum_ref.py), and with the LDS
kernels where they run: z, conv, status, iters, and post as int16."""
import functools

import numpy as np
import pytest

import ldpc_amd
import oracle
import qminsum_ref
import synth_graphs as sg
from ldpc_amd import _lib, ira
from ldpc_amd import montecarlo as mc

pytestmark = pytest.mark.gpu

SEED = 20260213
KERNELS = {"flooding": "phys_qcn_tile_kernel", "layered": "phys_qlayer_tile_kernel"}
SCHEDULES = ("flooding", "layered")
_SCHED = {"flooding": _lib.LDPC_SCHED_FLOODING, "layered": _lib.LDPC_SCHED_LAYERED}


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _assert_equal(got, want, what):
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")
    assert got["post"].dtype == np.int16 and want["post"].dtype == np.int16
    assert np.array_equal(got["post"], want["post"]), \
        f"{what}: {int((np.asarray(got['post']) != want['post']).sum())} posteriors differ"


def _graph(H):
    from ldpc_amd.device import Graph
    return Graph.cached(H)


def _kw(cn, qbits, scale, param_q):
    """phys_decode's float alpha / beta for the integer parameter."""
    return dict(cn=cn, qbits=qbits, llr_scale=scale, **({"alpha": param_q / 16.0} if cn == "nms"
                                                        else {"beta": param_q / scale}))


# ---- 1. every row-shape variant
@functools.lru_cache(maxsize=None)
def _deg16_ref(schedule, qbits, scale):
    return _frozen(qminsum_ref.decode(sg.graph("deg16"), sg.frames("deg16"), 10, "nms", schedule, qbits, scale,
                                      sg.ALPHA_Q))


def _shape_cases():
    """(graph, rule, schedule, qbits, scale, param_q, both exits wanted)"""
    out = []
    for name in sg.NAMES:
        if name == "pairs":
            continue
        out += [(name, cn, sch, sg.QBITS, sg.QSCALE, pq, True) for cn, sch, pq in sg.Q_CASES]
    out.append((sg.Q_OMS_GRAPH, "oms", "flooding", sg.QBITS, sg.QSCALE, sg.BETA_Q, True))
    out += [(name, "oms", "layered", sg.QBITS, sg.QSCALE, sg.BETA_Q, True) for name in ("longrow", "widecol")]
    for sch in SCHEDULES:
        out += [("deg16", "nms", sch, 5, 2.0, sg.ALPHA_Q, True), ("deg16", "nms", sch, 8, 8.0, sg.ALPHA_Q, True)]
    out.append(("deg16", "nms", "flooding", 4, 1.0, sg.ALPHA_Q, True))
    out.append(("deg16", "nms", "layered", 4, 1.0, sg.ALPHA_Q, False))  # no frame converges: equality only
    return out


@pytest.mark.parametrize("name,cn,schedule,qbits,scale,param_q,exits", _shape_cases())
def test_row_shapes_equal_restatement(gpu_available, name, cn, schedule, qbits, scale, param_q, exits):
    """kDeg 8 / 16 / 32 and the long-row loop (longrow), the column loop for any
    degree (widecol), a layer of more than 256 rows (widelayer), ragged m and
    n, a column with no edges; 70 noisy frames and the hand-made one: a full
    tile and a ragged one."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    if (qbits, scale) == (sg.QBITS, sg.QSCALE):
        want = sg.q_ref(name, cn, schedule, param_q)
    else:
        want = _deg16_ref(schedule, qbits, scale)
    if exits:
        assert sg.both_exits(want)
    g = _graph(sg.graph(name))
    kw = _kw(cn, qbits, scale, param_q)
    assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=qbits, qtile=True) == KERNELS[schedule]
    got = phys_decode(g, sg.frames(name), 10, post=True, schedule=schedule, qtile=True, **kw)
    _assert_equal(got, want, f"{name} {cn} {schedule} q{qbits}")


# ---- 2. tile == LDS == restatement
@functools.lru_cache(maxsize=None)
def _wimax():
    edd = ldpc_amd.load_committed_code("wimax_576_0.5")
    _, _, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(-2.5), 0, 96)  # test_gpu_qminsum.py's
    llr.setflags(write=False)
    return edd.physical_matrix(), llr


@functools.lru_cache(maxsize=None)
def _wimax_ref(T, cn, schedule, param_q, first=None):
    Hp, llr = _wimax()
    return _frozen(qminsum_ref.decode(Hp, llr if first is None else llr[:first], T, cn, schedule, 6, 4.0, param_q))


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("cn,param_q", [("nms", 12), ("oms", 2)])
def test_tile_equals_lds_equals_restatement(gpu_available, cn, param_q, schedule):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = _wimax_ref(20, cn, schedule, param_q)
    assert (want["status"] == 0).sum() >= 3 and (want["status"] != 0).sum() >= 3
    if (cn, schedule) == ("oms", "flooding"):
        assert want["counts"]["post_clamps"] > 0  # the posterior clamp bites
    Hp, llr = _wimax()
    g, kw = _graph(Hp), _kw(cn, 6, 4.0, param_q)
    assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=6) in ("phys_quant_kernel", "phys_quant_reg_kernel")
    assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=6, qtile=True) == KERNELS[schedule]
    lds = phys_decode(g, llr, 20, post=True, schedule=schedule, **kw)
    tile = phys_decode(g, llr, 20, post=True, schedule=schedule, qtile=True, **kw)
    _assert_equal(tile, want, f"{cn} {schedule} tile")
    _assert_equal(tile, lds, f"{cn} {schedule} tile vs LDS")


# ---- 3. edges of the batch
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_one_iteration(gpu_available, schedule):
    from ldpc_amd.device import phys_decode
    Hp, llr = _wimax()
    got = phys_decode(_graph(Hp), llr, 1, post=True, schedule=schedule, qtile=True, **_kw("nms", 6, 4.0, 12))
    want = _wimax_ref(1, "nms", schedule, 12)
    assert (want["iters"] == 1).all()
    _assert_equal(got, want, f"T = 1 {schedule}")


@pytest.mark.parametrize("schedule", SCHEDULES)
@pytest.mark.parametrize("count", [1, 65])
def test_one_frame_and_a_second_tile_of_one(gpu_available, count, schedule):
    from ldpc_amd.device import phys_decode
    Hp, llr = _wimax()
    got = phys_decode(_graph(Hp), llr[:count], 20, post=True, schedule=schedule, qtile=True,
                      **_kw("oms", 6, 4.0, 2))
    _assert_equal(got, _wimax_ref(20, "oms", schedule, 2, first=count), f"{count} frames {schedule}")


@pytest.mark.parametrize("schedule,converged", [("flooding", 292), ("layered", 286)])
def test_across_the_1024_frame_chunk(gpu_available, schedule, converged):
    """1030 frames of `ragged` (n = 101): a chunk of 1024 and one of 6."""
    from ldpc_amd.device import phys_decode
    llr = sg.frames("ragged", 1030, False)
    want = qminsum_ref.decode(sg.graph("ragged"), llr, 10, "nms", schedule, sg.QBITS, sg.QSCALE, sg.ALPHA_Q)
    assert int((want["status"] == 0).sum()) == converged
    got = phys_decode(_graph(sg.graph("ragged")), llr, 10, post=True, schedule=schedule, qtile=True,
                      **_kw("nms", sg.QBITS, sg.QSCALE, sg.ALPHA_Q))
    _assert_equal(got, want, f"1030 frames {schedule}")


@pytest.mark.parametrize("schedule", SCHEDULES)
def test_device_pointers(gpu_available, schedule):
    """LDPC_F_DEVICE_PTRS | LDPC_F_QUANT_TILE: inputs and outputs on the device."""
    from test_gpu_device_ptrs import DevBuf, Hip
    hip = Hip()
    Hp, llr = _wimax()
    g, want = _graph(Hp), _wimax_ref(20, "nms", schedule, 12)
    B, n = llr.shape
    d_llr = DevBuf.of(hip, np.array(llr))
    z, post = DevBuf(hip, (B, n), np.uint8, fill=7), DevBuf(hip, (B, n), np.int16, fill=-999)
    conv, status, iters = (DevBuf(hip, (B,), np.int32, fill=-7) for _ in range(3))
    rc = _lib.gpu().ldpc_phys_decode_q(g.handle, B, d_llr.data_ptr(), 20,
                                       _lib.LDPC_F_DEVICE_PTRS | _lib.LDPC_F_QUANT_TILE, _lib.LDPC_CN_NMS,
                                       _SCHED[schedule], 6, 4.0, 12, z.data_ptr(), conv.data_ptr(),
                                       status.data_ptr(), iters.data_ptr(), post.data_ptr(), None)
    _lib.check("ldpc_phys_decode_q", rc)
    hip.ok(hip.rt.hipDeviceSynchronize(), "hipDeviceSynchronize")
    got = dict(z=z.numpy(), conv=conv.numpy(), status=status.numpy(), iters=iters.numpy(), post=post.numpy())
    _assert_equal(got, want, f"device pointers {schedule}")


# ---- 4. the automatic path: the DVB-S2 profile, no flag
# (schedule, llr_scale, SNR dB, frames of 16 the restatement converges).  With
# llr_scale 4 the layered contract converges no frame of this code near its
# waterfall (the posterior is capped at 2 Qmax), hence scale 2 there.
DVB = [("layered", 2.0, -2.4, 8), ("flooding", 4.0, -2.0, 14)]


@pytest.mark.parametrize("schedule,scale,snr,converged", DVB)
def test_dvbs2_profile_runs_in_fixed_point_without_a_flag(gpu_available, schedule, scale, snr, converged):
    """A frame's quantized state (227 KB of messages + 130 KB of posteriors) does
    not fit LDS: the tile kernels are chosen by themselves.  (Before the tile
    path existed this call was LDPC_ERANGE.)"""
    from ldpc_amd.device import Graph, phys_decode, phys_kernel_name
    H = ira.dvbs2_profile_matrix()
    _, _, llr = oracle.generate_frames(H, SEED, 0, mc.sigma_for_snr(snr), 0, 16, ira=True)
    want = qminsum_ref.decode(H, llr, 30, "nms", schedule, 6, scale, 12)
    ok = int((want["status"] == 0).sum())
    assert ok >= 2 and 16 - ok >= 2
    assert ok == converged
    if schedule == "flooding":
        assert want["counts"]["post_clamps"] > 1000000
    g = Graph(H)
    assert phys_kernel_name(g, cn="nms", schedule=schedule, qbits=6) == KERNELS[schedule]
    got = phys_decode(g, llr, 30, post=True, schedule=schedule, **_kw("nms", 6, scale, 12))
    _assert_equal(got, want, f"dvbs2 profile {schedule}")


# ---- 5. Monte-Carlo
IDX = [0, 1, 2, 3, 4, 6]
# (schedule, SNR pair, failures of 256 at the first point, running count at a poll of the second)
MC_POINTS = [("flooding", (-2.5, -2.0), 229, 58), ("layered", (-1.5, -1.0), 77, 41)]


@pytest.mark.parametrize("schedule,snrs,failures,compacts_at", MC_POINTS)
def test_monte_carlo_counters(gpu_available, monkeypatch, schedule, snrs, failures, compacts_at):
    from ldpc_amd.device import Decoder, Graph
    H, T, B = ira.small_ira_matrix(), 20, 256
    g = Graph.cached(H)
    dec = Decoder(g, B)
    sig = [mc.sigma_for_snr(s) for s in snrs]
    want = []
    for p in range(len(sig)):
        u, llr = dec.generate(SEED, p, sig[p], 0, B)
        o = qminsum_ref.decode(H, llr, T, "nms", schedule, 6, 4.0, 12)
        want.append(oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])[IDX])
        if p == 1:
            # frames still running when the host polls after iteration `it`
            # (it < 4, then every 4th): at one of them between 1 and B / 4, so
            # that the run compacts
            polls = [it for it in range(T - 1) if it < 4 or (it + 1) % 4 == 0]
            running = [int(((o["conv"] < 0) | (o["conv"] > it)).sum()) for it in polls]
            assert any(1 <= r <= B // 4 for r in running), running
            assert compacts_at in running, running
    want = np.array(want)
    assert 0 < want[0][1] < B  # both exits at the first point
    assert int(want[0][1]) == failures

    def run(**kw):
        return dec.phys_mc_run(g, SEED, sig, B, 0, T, cn="nms", schedule=schedule, alpha=0.75, qbits=6, llr_scale=4.0,
                               **kw)[:, IDX]
    tile = run(qtile=True)
    np.testing.assert_array_equal(tile, want, err_msg="tile vs restatement")
    np.testing.assert_array_equal(run(), tile, err_msg="LDS vs tile")
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")
    np.testing.assert_array_equal(run(qtile=True), tile, err_msg="without compaction")
    monkeypatch.delenv("LDPC_PHYS_COMPACT")
    res, ctr = mc.simulate("ira_1440_0.5", list(snrs), B, T, seed=SEED, mode="physical", cn_rule="nms",
                           schedule=schedule, alpha=0.75, qbits=6, llr_scale=4.0, quant_tile=True)
    assert res.config.decoder_type == mc.decoder_type("nms", schedule, 6)
    np.testing.assert_array_equal(ctr[:, IDX], want)
    assert [sp.failed_blocks for sp in res.snr_points] == [int(w[1]) for w in want]


# ---- 6. refusals
def test_refusals(gpu_available):
    Hp, frames = _wimax()
    g, llr = _graph(Hp), np.ascontiguousarray(frames[:4])
    L = _lib.gpu()
    z = np.empty((4, g.n), np.uint8)
    ctr = np.zeros((1, _lib.LDPC_MC_NCOUNT), np.int64)
    sig = np.array([1.0])
    F_Q, F_HBM, F_TILE = _lib.LDPC_F_QUANT_TILE, _lib.LDPC_F_PHYS_HBM, _lib.LDPC_F_LAYERED_TILE
    NMS, LAYERED = _lib.LDPC_CN_NMS, _lib.LDPC_SCHED_LAYERED
    from ldpc_amd.device import Decoder, Graph
    edd = ldpc_amd.load_committed_code("wimax_576_0.5")
    dec = Decoder(Graph.cached(edd._h_std), 64)
    import ctypes
    sp = sig.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cp = ctr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    # the four fp32 entries do not know the flag
    calls = {
        "ldpc_phys_decode": lambda: L.ldpc_phys_decode(g.handle, 4, _lib.ptr(llr), 5, F_Q, _lib.ptr(z), None, None,
                                                       None, None, None),
        "ldpc_phys_decode_ex": lambda: L.ldpc_phys_decode_ex(g.handle, 4, _lib.ptr(llr), 5, F_Q, NMS, LAYERED, 0.75,
                                                             _lib.ptr(z), None, None, None, None, None),
        "ldpc_phys_mc_run": lambda: L.ldpc_phys_mc_run(dec._h, g.handle, SEED, 1, sp, 4, 0, 5, F_Q, cp, None),
        "ldpc_phys_mc_run_ex": lambda: L.ldpc_phys_mc_run_ex(dec._h, g.handle, SEED, 1, sp, 4, 0, 5, F_Q, NMS,
                                                             LAYERED, 0.75, cp, None),
    }
    for fn, call in calls.items():
        assert call() == _lib.LDPC_EINVAL, fn
        msg = _lib.lib().ldpc_last_error()
        assert b"LDPC_F_QUANT_TILE" in msg and fn.encode() in msg, msg
    assert L.ldpc_phys_kernel_name_ex(g.handle, F_Q, NMS, LAYERED) == b""
    assert L.ldpc_phys_kernel_name(g.handle, F_Q) == b""
    # the fp32 tile flags stay refused on the fixed-point entries, with or without the new one
    for flags, named in ((F_HBM | F_Q, b"LDPC_F_PHYS_HBM"), (F_TILE | F_Q, b"LDPC_F_LAYERED_TILE")):
        for sched in (_lib.LDPC_SCHED_FLOODING, LAYERED):
            rc = L.ldpc_phys_decode_q(g.handle, 4, _lib.ptr(llr), 5, flags, NMS, sched, 6, 4.0, 12, _lib.ptr(z), None,
                                      None, None, None, None)
            assert rc == _lib.LDPC_ERANGE and named in _lib.lib().ldpc_last_error()
            rc = L.ldpc_phys_mc_run_q(dec._h, g.handle, SEED, 1, sp, 4, 0, 5, flags, NMS, sched, 6, 4.0, 12, cp, None)
            assert rc == _lib.LDPC_ERANGE and named in _lib.lib().ldpc_last_error()
            assert L.ldpc_phys_kernel_name_q(g.handle, flags, NMS, sched, 6) == b""
    # and the argument checks still come first
    rc = L.ldpc_phys_decode_q(g.handle, 4, _lib.ptr(llr), 5, F_Q, NMS, LAYERED, 9, 4.0, 12, _lib.ptr(z), None, None,
                              None, None, None)
    assert rc == _lib.LDPC_EINVAL and b"qbits" in _lib.lib().ldpc_last_error()
    assert L.ldpc_phys_kernel_name_q(g.handle, F_Q, NMS, LAYERED, 9) == b""
