"""Physical mode's fixed-point min-sum decoder (q-bit messages) on the GPU.
The contract is all-integer after the load, so every output must EQUAL the
numpy int32 restatement (tests/qminsum_ref.py) for every frame: z, conv,
status, iters and the int16 posteriors."""
import functools

import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import oracle
import qminsum_ref
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc

SEED = 20260213
SCHEDULES = ("flooding", "layered")


@functools.lru_cache(maxsize=None)
def _code(name):
    edd = ldpc_amd.load_committed_code(name)
    return edd, edd.physical_matrix()


@functools.lru_cache(maxsize=None)
def _frames(name, snr, count):
    edd, _ = _code(name)
    u, c, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(snr), 0, count)
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def _ref(name, snr, count, T, cn, schedule, qbits, scale, param_q, first=None):
    """The restatement's result, computed once and shared (read-only)."""
    llr = _frames(name, snr, count)
    r = qminsum_ref.decode(_code(name)[1], llr if first is None else llr[:first], T, cn, schedule, qbits, scale,
                           param_q)
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _graph(name):
    from ldpc_amd.device import Graph
    return Graph.cached(_code(name)[1])


def _kw(cn, qbits, scale, param_q):
    """phys_decode's float alpha / beta for the integer parameter."""
    return dict(cn=cn, qbits=qbits, llr_scale=scale, **({"alpha": param_q / 16.0} if cn == "nms"
                                                        else {"beta": param_q / scale}))


def _assert_equal(got, want, what):
    for key in ("z", "conv", "status", "iters"):
        assert np.array_equal(got[key], want[key]), \
            f"{what}: {key} differs in {int((np.asarray(got[key]) != want[key]).sum())} places"
    assert got["post"].dtype == np.int16 and want["post"].dtype == np.int16
    assert np.array_equal(got["post"], want["post"]), \
        f"{what}: {int((got['post'] != want['post']).sum())} posteriors differ"


# (code, snr, frames, T, rule, q, scale, param_q)
BASE = [
    ("wimax_576_0.5", -2.5, 96, 20, "nms", 6, 4.0, 12),
    ("wimax_576_0.5", -2.5, 96, 20, "oms", 6, 4.0, 2),
    ("wimax_576_0.5", -2.5, 96, 20, "nms", 5, 2.0, 12),
    ("wimax_576_0.5", -2.5, 96, 20, "nms", 8, 8.0, 12),
    ("wimax_2304_0.5", -2.5, 96, 20, "nms", 6, 4.0, 12),
    ("wimax_2304_0.75A", -1.0, 96, 20, "nms", 6, 4.0, 12),  # row degree 14-15
    ("wimax_2304_0.75A", -1.0, 96, 20, "oms", 6, 4.0, 2),
    ("BCH_7_4_1_strip", 2.0, 256, 10, "nms", 6, 4.0, 12),
    ("BCH_7_4_1_strip", 2.0, 256, 10, "nms", 4, 1.0, 12),
]
CASES = [c + (s,) for c in BASE for s in SCHEDULES]


@pytest.mark.gpu
@pytest.mark.parametrize("name,snr,count,T,cn,qbits,scale,param_q,schedule", CASES)
def test_bit_exact_against_restatement(gpu_available, name, snr, count, T, cn, qbits, scale, param_q, schedule):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = _ref(name, snr, count, T, cn, schedule, qbits, scale, param_q)
    if not name.startswith("BCH"):  # both exits are exercised
        assert (want["status"] == 0).sum() >= 3 and (want["status"] != 0).sum() >= 3
    if schedule == "layered":
        assert want["counts"]["post_clamps"] == 0
    g = _graph(name)
    # flooding on the graphs with rows of up to 8 edges: the kernel with its indices in registers
    reg = schedule == "flooding" and name != "wimax_2304_0.75A"
    assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=qbits) == \
        ("phys_quant_reg_kernel" if reg else "phys_quant_kernel")
    got = phys_decode(g, _frames(name, snr, count), T, post=True, schedule=schedule, **_kw(cn, qbits, scale, param_q))
    _assert_equal(got, want, f"{name} {cn} {schedule} q{qbits}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,snr,count,T,cn,qbits,scale,param_q", [BASE[0], BASE[1], BASE[4], BASE[8]])
def test_generic_kernel_forced(gpu_available, monkeypatch, name, snr, count, T, cn, qbits, scale, param_q):
    """LDPC_PHYS_Q_REG=0: the flooding schedule through the generic byte-addressed
    kernel (any degree), the same integers."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    g = _graph(name)
    monkeypatch.setenv("LDPC_PHYS_Q_REG", "0")
    assert phys_kernel_name(g, cn=cn, qbits=qbits) == "phys_quant_kernel"
    got = phys_decode(g, _frames(name, snr, count), T, post=True, **_kw(cn, qbits, scale, param_q))
    _assert_equal(got, _ref(name, snr, count, T, cn, "flooding", qbits, scale, param_q), f"generic {name} {cn}")


@pytest.mark.gpu
def test_cases_exercise_every_saturation():
    """Asserted on the restatement alone: across the cases the quantizer
    saturates at the load, the Q clamp and the posterior clamp bite, and
    posteriors equal to 0 occur; the posterior clamp only in flooding cases.
    (Marked gpu to run beside the cases above, whose cached references it reads.)"""
    tot = dict(lam_sat=0, q_clamps=0, post_clamps=0, post_zero=0)
    for name, snr, count, T, cn, qbits, scale, param_q, schedule in CASES:
        c = _ref(name, snr, count, T, cn, schedule, qbits, scale, param_q)["counts"]
        for k in tot:
            tot[k] += c[k]
        if schedule == "layered":
            assert c["post_clamps"] == 0, (name, cn, qbits)
    assert all(v > 0 for v in tot.values()), tot
    assert _ref("wimax_576_0.5", -2.5, 96, 20, "oms", "flooding", 6, 4.0, 2)["counts"]["post_clamps"] > 0


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_one_iteration_and_single_frame(gpu_available, schedule):
    from ldpc_amd.device import phys_decode
    name, snr = "wimax_576_0.5", -2.5
    g, llr = _graph(name), _frames(name, snr, 96)
    got = phys_decode(g, llr, 1, post=True, schedule=schedule, **_kw("nms", 6, 4.0, 12))
    _assert_equal(got, _ref(name, snr, 96, 1, "nms", schedule, 6, 4.0, 12), f"T=1 {schedule}")
    got = phys_decode(g, llr[:1], 20, post=True, schedule=schedule, **_kw("oms", 6, 4.0, 2))
    _assert_equal(got, _ref(name, snr, 96, 20, "oms", schedule, 6, 4.0, 2, first=1), f"one frame {schedule}")


@pytest.mark.gpu
@pytest.mark.parametrize("schedule,reg", [("flooding", "1"), ("flooding", "0"), ("layered", "1")])
def test_lds_reuse_one_workgroup_many_frames(gpu_available, monkeypatch, schedule, reg):
    """8 workgroups for 96 frames: each decodes 12 in sequence in the same LDS
    (flooding: the register kernel and, forced, the generic one)."""
    from ldpc_amd.device import phys_decode
    monkeypatch.setenv("LDPC_PHYS_Q_GRID", "8")
    monkeypatch.setenv("LDPC_PHYS_Q_REG", reg)
    name, snr = "wimax_576_0.5", -2.5
    got = phys_decode(_graph(name), _frames(name, snr, 96), 20, post=True, schedule=schedule,
                      **_kw("nms", 6, 4.0, 12))
    _assert_equal(got, _ref(name, snr, 96, 20, "nms", schedule, 6, 4.0, 12), f"grid 8 {schedule}")


def _raw_decode(g, llr, cn, sched, qbits, scale, param_q, flags=0):
    llr = np.ascontiguousarray(llr)
    z = np.empty(llr.shape, np.uint8)
    return _lib.gpu().ldpc_phys_decode_q(g.handle, len(llr), _lib.ptr(llr), 5, flags, cn, sched, qbits, scale, param_q,
                                         _lib.ptr(z), None, None, None, None, None)


@pytest.mark.gpu
def test_unsupported_combinations(gpu_available):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    name = "wimax_576_0.5"
    g, llr = _graph(name), _frames(name, -2.5, 96)[:4]
    NMS, OMS, SPA = _lib.LDPC_CN_NMS, _lib.LDPC_CN_OMS, _lib.LDPC_CN_SPA
    for schedule in SCHEDULES:
        with pytest.raises(ldpc_amd.LdpcError) as e:
            phys_decode(g, llr, 5, cn="nms", schedule=schedule, hbm=True, qbits=6)
        assert e.value.code == _lib.LDPC_ERANGE and "LDPC_F_PHYS_HBM" in str(e.value)
        assert phys_kernel_name(g, hbm=True, cn="nms", schedule=schedule, qbits=6) == ""
    assert _raw_decode(g, llr, SPA, 0, 6, 4.0, 12) == _lib.LDPC_EINVAL
    assert b"cn_rule" in _lib.lib().ldpc_last_error()
    for what, cn, sched, qbits, scale, param_q in (
            ("qbits", NMS, 0, 3, 4.0, 12), ("qbits", NMS, 1, 9, 4.0, 12), ("llr_scale", NMS, 0, 6, 0.0, 12),
            ("llr_scale", OMS, 1, 6, float("inf"), 2), ("param_q", NMS, 0, 6, 4.0, 17),
            ("param_q", NMS, 1, 6, 4.0, 0), ("param_q", OMS, 0, 6, 4.0, 32), ("param_q", OMS, 0, 4, 1.0, 8),
            ("schedule", NMS, 2, 6, 4.0, 12), ("cn_rule", 3, 0, 6, 4.0, 12)):
        assert _raw_decode(g, llr, cn, sched, qbits, scale, param_q) == _lib.LDPC_EINVAL, (what, qbits, param_q)
        assert what.encode() in _lib.lib().ldpc_last_error(), (what, _lib.lib().ldpc_last_error())
    L = _lib.gpu()
    for cn, sched, qbits, flags in ((SPA, 0, 6, 0), (NMS, 0, 3, 0), (NMS, 1, 9, 0), (NMS, 2, 6, 0),
                                    (OMS, 0, 6, _lib.LDPC_F_PHYS_HBM)):
        assert L.ldpc_phys_kernel_name_q(g.handle, flags, cn, sched, qbits) == b"", (cn, sched, qbits, flags)
    for cn in (NMS, OMS):
        for sched in (0, 1):
            for qbits in (4, 8):
                assert L.ldpc_phys_kernel_name_q(g.handle, 0, cn, sched, qbits) in \
                    (b"phys_quant_reg_kernel", b"phys_quant_kernel")
    # int8 E in rows padded to 4 bytes, int16 L (n + 1 entries, padded to 4 bytes), int8 Lam (flooding only)
    Hp = _code(name)[1]
    epad = int(((np.diff(Hp.indptr) + 3) // 4 * 4).sum())
    assert g.n % 4 == 0
    assert L.ldpc_phys_q_lds_bytes(g.handle, 0) == epad + 2 * g.n + 4 + g.n
    assert L.ldpc_phys_q_lds_bytes(g.handle, 1) == epad + 2 * g.n + 4
    assert L.ldpc_phys_q_lds_bytes(g.handle, 2) == -1


@pytest.mark.gpu
def test_row_of_one_edge_is_einval(gpu_available):
    from ldpc_amd.device import Graph
    g = Graph(np.array([[1, 1, 0], [0, 0, 1]]))
    assert _raw_decode(g, np.zeros((1, 3)), _lib.LDPC_CN_NMS, 0, 6, 4.0, 12) == _lib.LDPC_EINVAL
    assert b"at least 2 edges" in _lib.lib().ldpc_last_error()
    assert _lib.gpu().ldpc_phys_kernel_name_q(g.handle, 0, _lib.LDPC_CN_NMS, 0, 6) == b""


@pytest.mark.gpu
def test_device_pointers(gpu_available):
    """LDPC_F_DEVICE_PTRS: inputs and outputs on the device, same results."""
    from test_gpu_device_ptrs import DevBuf, Hip
    hip = Hip()
    name, snr = "wimax_576_0.5", -2.5
    g, llr = _graph(name), _frames(name, snr, 96)
    want = _ref(name, snr, 96, 20, "nms", "layered", 6, 4.0, 12)
    B, n = llr.shape
    d_llr = DevBuf.of(hip, np.array(llr))
    z, post = DevBuf(hip, (B, n), np.uint8, fill=7), DevBuf(hip, (B, n), np.int16, fill=-999)
    conv, status, iters = (DevBuf(hip, (B,), np.int32, fill=-7) for _ in range(3))
    rc = _lib.gpu().ldpc_phys_decode_q(g.handle, B, d_llr.data_ptr(), 20, _lib.LDPC_F_DEVICE_PTRS, _lib.LDPC_CN_NMS,
                                       _lib.LDPC_SCHED_LAYERED, 6, 4.0, 12, z.data_ptr(), conv.data_ptr(),
                                       status.data_ptr(), iters.data_ptr(), post.data_ptr(), None)
    _lib.check("ldpc_phys_decode_q", rc)
    hip.ok(hip.rt.hipDeviceSynchronize(), "hipDeviceSynchronize")
    got = dict(z=z.numpy(), conv=conv.numpy(), status=status.numpy(), iters=iters.numpy(), post=post.numpy())
    _assert_equal(got, want, "device pointers")


@pytest.mark.gpu
def test_monte_carlo_counters_equal_restatement(gpu_available):
    """The on-device Lambda is -(float)llr of the same fp64 value, so the
    counters are EQUAL to the restatement's on the frames generate() returns."""
    from ldpc_amd.device import Decoder, Graph
    name, T, B = "wimax_576_0.5", 20, 256
    edd, Hp = _code(name)
    dec = Decoder(Graph.cached(edd._h_std), B)
    gp = _graph(name)
    snrs = (-2.5, 0.0)
    sig = [mc.sigma_for_snr(s) for s in snrs]
    frames = [dec.generate(SEED, p, sig[p], 0, B) for p in range(len(sig))]
    want = {}
    for schedule in ("layered", "flooding"):
        got = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", schedule=schedule, alpha=0.75, qbits=6, llr_scale=4.0)
        for p, (u, llr) in enumerate(frames):
            o = qminsum_ref.decode(Hp, llr, T, "nms", schedule, 6, 4.0, 12)
            w = oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])
            want[schedule, p] = w
            np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w[[0, 1, 2, 3, 4, 6]],
                                          err_msg=f"{schedule} point {p}")
        assert 1 <= want[schedule, 0][1] <= B - 1 and want[schedule, 1][1] == 0  # waterfall, then error-free
    res, ctr = mc.simulate(name, list(snrs), B, T, seed=SEED, mode="physical", cn_rule="nms", schedule="layered",
                           alpha=0.75, qbits=6, llr_scale=4.0)
    assert res.config.decoder_type == "minsum-normalized-layered-q6"
    for p, sp in enumerate(res.snr_points):
        w = want["layered", p]
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w[[0, 1, 2, 3, 4, 6]])
        assert (sp.total_blocks, sp.failed_blocks) == (B, int(w[1]))


@pytest.mark.gpu
def test_defaults_keep_the_fp32_path(gpu_available):
    from ldpc_amd.device import phys_decode
    name, snr = "wimax_576_0.5", -2.5
    got = phys_decode(_graph(name), _frames(name, snr, 96), 20, post=True, cn="nms")
    want = minsum_ref.decode(_code(name)[1], _frames(name, snr, 96), 20, "nms", "flooding", 0.75, 0.5)
    assert got.post.dtype == np.float32 and np.array_equal(got.post, want["post"])
