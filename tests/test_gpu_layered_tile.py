"""The layered min-sum schedule with the decoder state in HBM
(phys_layer_tile_kernel, csrc/phys_tile.hip): forced with tile=True
(LDPC_F_LAYERED_TILE) where the state fits LDS, automatic on the DVB-S2
profile (n = 64800), whose layered state does not fit.

Min-sum in fp32 without FMA contraction has one result, so every comparison is
EQUALITY: with the numpy restatement (tests/minsum_ref.py), and with the LDS
kernel where that runs -- z, conv, status, iters, and post as bit patterns."""
import functools

import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import oracle
import synth_graphs as sg
from ldpc_amd import _lib, ira
from ldpc_amd import montecarlo as mc

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
KERNEL = "phys_layer_tile_kernel"


def _frozen(r):
    for v in r.values():
        v.setflags(write=False)
    return r


def _assert_equal(got, want, what):
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")
    assert got["post"].dtype == np.float32 and want["post"].dtype == np.float32
    a, b = np.asarray(got["post"]).view(np.uint32), np.asarray(want["post"]).view(np.uint32)
    assert np.array_equal(a, b), f"{what}: {int((a != b).sum())} posteriors differ in their bits"


def _graph(H):
    from ldpc_amd.device import Graph
    return Graph.cached(H)


# ---- 1. every row-shape variant
@pytest.mark.parametrize("name", [n for n in sg.NAMES if n != "pairs"])
def test_row_shapes_equal_restatement(gpu_available, name):
    """kDeg 8 / 16 / 32, the long-row loop (longrow), a layer of more than 256
    rows (widelayer), ragged m and n, a column with no edges; 70 noisy frames
    and the hand-made one: a full tile and a ragged one."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    cn = sg.LAYERED_RULE[name]
    want = sg.ms_ref(name, cn, "layered")
    assert sg.both_exits(want)
    g = _graph(sg.graph(name))
    assert phys_kernel_name(g, cn=cn, schedule="layered", tile=True) == KERNEL
    got = phys_decode(g, sg.frames(name), 10, post=True, cn=cn, schedule="layered", alpha=sg.ALPHA, beta=sg.BETA,
                      tile=True)
    _assert_equal(got, want, f"{name} {cn}")


# ---- 2. tile == LDS == restatement
IRA_SNR = -2.5  # within the allowed [-2.7, -2.2]: the Philox frames split well inside the condition (asserted)


@functools.lru_cache(maxsize=None)
def _code(name):
    if name == "ira":
        return ira.small_ira_matrix()
    return ldpc_amd.load_committed_code(name).physical_matrix()


@functools.lru_cache(maxsize=None)
def _frames(name, count=96):
    if name == "ira":
        _, _, llr = oracle.generate_frames(_code("ira"), SEED, 2, mc.sigma_for_snr(IRA_SNR), 0, count, ira=True)
    else:  # the recipe of test_gpu_minsum.py
        edd = ldpc_amd.load_committed_code(name)
        _, _, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(-2.5), 0, count)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _ref(name, T, cn, count=96, first=None):
    llr = _frames(name, count)
    return _frozen(minsum_ref.decode(_code(name), llr if first is None else llr[:first], T, cn, "layered", ALPHA, BETA))


@pytest.mark.parametrize("name,cn", [("ira", "nms"), ("ira", "oms"), ("wimax_576_0.5", "nms"),
                                     ("wimax_576_0.5", "oms")])
def test_tile_equals_lds_equals_restatement(gpu_available, name, cn):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = _ref(name, 20, cn)
    assert (want["status"] == 0).sum() >= 3 and (want["status"] != 0).sum() >= 3
    g, llr = _graph(_code(name)), _frames(name)
    assert phys_kernel_name(g, cn=cn, schedule="layered") == "phys_layered_kernel"
    assert phys_kernel_name(g, cn=cn, schedule="layered", tile=True) == KERNEL
    lds = phys_decode(g, llr, 20, post=True, cn=cn, schedule="layered", alpha=ALPHA, beta=BETA)
    tile = phys_decode(g, llr, 20, post=True, cn=cn, schedule="layered", alpha=ALPHA, beta=BETA, tile=True)
    _assert_equal(tile, want, f"{name} {cn} tile")
    _assert_equal(tile, lds, f"{name} {cn} tile vs LDS")


# ---- 3. edges of the batch
def test_one_iteration(gpu_available):
    from ldpc_amd.device import phys_decode
    got = phys_decode(_graph(_code("ira")), _frames("ira"), 1, post=True, cn="nms", schedule="layered", alpha=ALPHA,
                      tile=True)
    want = _ref("ira", 1, "nms")
    assert (want["iters"] == 1).all()
    _assert_equal(got, want, "T = 1")


@pytest.mark.parametrize("count", [1, 65])
def test_one_frame_and_a_second_tile_of_one(gpu_available, count):
    from ldpc_amd.device import phys_decode
    got = phys_decode(_graph(_code("ira")), _frames("ira")[:count], 20, post=True, cn="oms", schedule="layered",
                      beta=BETA, tile=True)
    _assert_equal(got, _ref("ira", 20, "oms", first=count), f"{count} frames")


def test_across_the_1024_frame_chunk(gpu_available):
    """1030 frames of `ragged` (n = 101): a chunk of 1024 and one of 6."""
    from ldpc_amd.device import phys_decode
    llr = sg.frames("ragged", 1030, False)
    want = minsum_ref.decode(sg.graph("ragged"), llr, 10, "nms", "layered", sg.ALPHA, sg.BETA)
    assert 3 <= (want["status"] == 0).sum() <= 1030 - 3
    got = phys_decode(_graph(sg.graph("ragged")), llr, 10, post=True, cn="nms", schedule="layered", alpha=sg.ALPHA,
                      tile=True)
    _assert_equal(got, want, "1030 frames")


def test_device_pointers(gpu_available):
    """LDPC_F_DEVICE_PTRS on the tile path: inputs and outputs on the device."""
    from test_gpu_device_ptrs import DevBuf, Hip
    hip = Hip()
    g, llr = _graph(_code("ira")), _frames("ira")
    want = _ref("ira", 20, "nms")
    B, n = llr.shape
    d_llr = DevBuf.of(hip, np.array(llr))
    z, post = DevBuf(hip, (B, n), np.uint8, fill=7), DevBuf(hip, (B, n), np.float32, fill=-999.0)
    conv, status, iters = (DevBuf(hip, (B,), np.int32, fill=-7) for _ in range(3))
    rc = _lib.gpu().ldpc_phys_decode_ex(g.handle, B, d_llr.data_ptr(), 20,
                                        _lib.LDPC_F_DEVICE_PTRS | _lib.LDPC_F_LAYERED_TILE, _lib.LDPC_CN_NMS,
                                        _lib.LDPC_SCHED_LAYERED, ALPHA, z.data_ptr(), conv.data_ptr(),
                                        status.data_ptr(), iters.data_ptr(), post.data_ptr(), None)
    _lib.check("ldpc_phys_decode_ex", rc)
    hip.ok(hip.rt.hipDeviceSynchronize(), "hipDeviceSynchronize")
    got = dict(z=z.numpy(), conv=conv.numpy(), status=status.numpy(), iters=iters.numpy(), post=post.numpy())
    _assert_equal(got, want, "device pointers")


# ---- 4. the automatic path: the DVB-S2 profile, no flag
# Both exits are wanted (at least 2 frames converge, at least 2 do not), at an
# SNR in [-2.2, -1.9].  numpy-generated frames split 13 / 3 at -2.0 dB; the
# project's Philox frames all converge at -2.0 and -2.1 dB and 15 of 16 at
# -2.15 dB, so the point is -2.2 dB: 14 converge in 13-19 iterations, 2 do not
# in 30 (asserted on the restatement below).
DVB_SNR = -2.2


def test_dvbs2_profile_runs_layered_without_a_flag(gpu_available):
    """A frame's layered state (E 0.9 MB + L 0.26 MB) does not fit LDS: the
    tile kernels are chosen by themselves.  (Before the tile path existed this
    call was LDPC_ERANGE.)"""
    from ldpc_amd.device import Graph, phys_decode, phys_kernel_name
    H = ira.dvbs2_profile_matrix()
    _, _, llr = oracle.generate_frames(H, SEED, 0, mc.sigma_for_snr(DVB_SNR), 0, 16, ira=True)
    want = minsum_ref.decode(H, llr, 30, "nms", "layered", ALPHA, BETA)
    assert (want["status"] == 0).sum() >= 2 and (want["status"] != 0).sum() >= 2
    g = Graph(H)
    assert phys_kernel_name(g, cn="nms", schedule="layered") == KERNEL
    got = phys_decode(g, llr, 30, post=True, cn="nms", schedule="layered", alpha=ALPHA)
    _assert_equal(got, want, "dvbs2 profile")


# ---- 5. Monte-Carlo
IDX = [0, 1, 2, 3, 4, 6]


def test_monte_carlo_counters(gpu_available, monkeypatch):
    from ldpc_amd.device import Decoder, Graph
    H, T, B = _code("ira"), 20, 256
    g = Graph.cached(H)
    dec = Decoder(g, B)
    snrs = (-2.5, -2.0)
    sig = [mc.sigma_for_snr(s) for s in snrs]
    want = []
    for p in range(len(sig)):
        u, llr = dec.generate(SEED, p, sig[p], 0, B)
        o = minsum_ref.decode(H, llr, T, "nms", "layered", ALPHA, BETA)
        want.append(oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])[IDX])
        if p == 1:
            # frames still running when the host polls after iteration `it`
            # (it < 4, then every 4th): at one of them between 1 and B / 4, so
            # that the run compacts
            polls = [it for it in range(T - 1) if it < 4 or (it + 1) % 4 == 0]
            running = [int(((o["conv"] < 0) | (o["conv"] > it)).sum()) for it in polls]
            assert any(1 <= r <= B // 4 for r in running), running
    want = np.array(want)
    assert 0 < want[0][1] < B  # both exits at the first point

    def run(**kw):
        return dec.phys_mc_run(g, SEED, sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA, **kw)[:, IDX]
    with pytest.raises(ValueError, match="layered"):
        dec.phys_mc_run(g, SEED, sig, B, 0, T, cn="nms", schedule="flooding", tile=True)
    tile = run(tile=True)
    np.testing.assert_array_equal(tile, want, err_msg="tile vs restatement")
    np.testing.assert_array_equal(run(), tile, err_msg="LDS vs tile")
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")
    np.testing.assert_array_equal(run(tile=True), tile, err_msg="without compaction")
    monkeypatch.delenv("LDPC_PHYS_COMPACT")
    res, ctr = mc.simulate("ira_1440_0.5", list(snrs), B, T, seed=SEED, mode="physical", cn_rule="nms",
                           schedule="layered", alpha=ALPHA, layered_tile=True)
    assert res.config.decoder_type == "minsum-normalized-layered"
    np.testing.assert_array_equal(ctr[:, IDX], want)
    assert [sp.failed_blocks for sp in res.snr_points] == [int(w[1]) for w in want]


# ---- 6. refusals
def test_refusals(gpu_available):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    g, llr = _graph(_code("wimax_576_0.5")), np.ascontiguousarray(_frames("wimax_576_0.5")[:4])
    for cn in ("spa", "nms"):
        with pytest.raises(ValueError, match="layered"):
            phys_decode(g, llr, 5, cn=cn, schedule="flooding", tile=True)
        with pytest.raises(ValueError, match="layered"):
            phys_kernel_name(g, cn=cn, schedule="flooding", tile=True)
    L = _lib.gpu()
    z = np.empty((4, g.n), np.uint8)
    F_TILE, F_HBM = _lib.LDPC_F_LAYERED_TILE, _lib.LDPC_F_PHYS_HBM

    def raw(flags, cn, sched, param):
        return L.ldpc_phys_decode_ex(g.handle, 4, _lib.ptr(llr), 5, flags, cn, sched, param, _lib.ptr(z), None, None,
                                     None, None, None)
    assert raw(F_TILE, _lib.LDPC_CN_NMS, _lib.LDPC_SCHED_FLOODING, ALPHA) == _lib.LDPC_EINVAL
    assert b"LDPC_F_LAYERED_TILE" in _lib.lib().ldpc_last_error()
    assert raw(F_TILE, _lib.LDPC_CN_SPA, _lib.LDPC_SCHED_FLOODING, 0.0) == _lib.LDPC_EINVAL
    assert L.ldpc_phys_decode(g.handle, 4, _lib.ptr(llr), 5, F_TILE, _lib.ptr(z), None, None, None, None,
                              None) == _lib.LDPC_EINVAL
    assert raw(F_TILE, _lib.LDPC_CN_SPA, _lib.LDPC_SCHED_LAYERED, 0.0) == _lib.LDPC_EINVAL
    for flags in (F_HBM, F_HBM | F_TILE):
        assert raw(flags, _lib.LDPC_CN_NMS, _lib.LDPC_SCHED_LAYERED, ALPHA) == _lib.LDPC_ERANGE
        msg = _lib.lib().ldpc_last_error()
        assert b"layered" in msg and b"LDPC_F_LAYERED_TILE" in msg
        assert L.ldpc_phys_kernel_name_ex(g.handle, flags, _lib.LDPC_CN_NMS, _lib.LDPC_SCHED_LAYERED) == b""
    assert L.ldpc_phys_kernel_name_ex(g.handle, F_TILE, _lib.LDPC_CN_NMS, _lib.LDPC_SCHED_FLOODING) == b""
    assert L.ldpc_phys_kernel_name_ex(g.handle, F_TILE, _lib.LDPC_CN_SPA, _lib.LDPC_SCHED_LAYERED) == b""
    # the fixed-point entries have no HBM path
    for sched in (_lib.LDPC_SCHED_FLOODING, _lib.LDPC_SCHED_LAYERED):
        rc = L.ldpc_phys_decode_q(g.handle, 4, _lib.ptr(llr), 5, F_TILE, _lib.LDPC_CN_NMS, sched, 6, 4.0, 12,
                                  _lib.ptr(z), None, None, None, None, None)
        assert rc == _lib.LDPC_ERANGE and b"LDPC_F_LAYERED_TILE" in _lib.lib().ldpc_last_error()
        assert L.ldpc_phys_kernel_name_q(g.handle, F_TILE, _lib.LDPC_CN_NMS, sched, 6) == b""
    with pytest.raises(ldpc_amd.LdpcError) as e:
        phys_decode(g, llr, 5, cn="nms", schedule="layered", tile=True, qbits=6)
    assert e.value.code == _lib.LDPC_ERANGE
