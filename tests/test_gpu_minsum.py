"""Physical mode's min-sum check rules (normalized, offset) and the layered
schedule on the GPU.  Min-sum in fp32 is subtract, abs, compare, one multiply
or subtract, add -- no transcendental, and the library is built without FMA
contraction -- so every output must EQUAL the numpy restatement
(tests/minsum_ref.py) for every frame: z, conv, status, iters and the
posteriors bit for bit.  (The sum-product test accepts 95 % frame agreement
because hardware exp/log differ from libm; nothing of that kind applies here.)"""
import functools

import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import oracle
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc

SEED = 20260213
ALPHA, BETA = 0.75, 0.5


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
def _ref(name, snr, count, T, cn, schedule, first=None):
    """The restatement's result, computed once and shared (read-only)."""
    llr = _frames(name, snr, count)
    r = minsum_ref.decode(_code(name)[1], llr if first is None else llr[:first], T, cn, schedule, ALPHA, BETA)
    for v in r.values():
        v.setflags(write=False)
    return r


def _graph(name):
    from ldpc_amd.device import Graph
    return Graph.cached(_code(name)[1])


def _assert_equal(got, want, what):
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(got[key], want[key], err_msg=f"{what}: {key}")
    assert got["post"].dtype == np.float32 and want["post"].dtype == np.float32
    assert np.array_equal(got["post"], want["post"]), \
        f"{what}: {int((got['post'] != want['post']).sum())} posteriors differ"


CASES = [(name, snr, 96, 20, cn, sch)
         for name, snr, rules in (("wimax_576_0.5", -2.5, ("nms", "oms")), ("wimax_2304_0.5", -2.5, ("nms",)),
                                  ("wimax_2304_0.75A", -1.0, ("nms", "oms")))
         for cn in rules for sch in ("flooding", "layered")]
CASES += [("BCH_7_4_1_strip", 2.0, 256, 10, "nms", sch) for sch in ("flooding", "layered")]


@pytest.mark.gpu
@pytest.mark.parametrize("name,snr,count,T,cn,schedule", CASES)
def test_bit_exact_against_restatement(gpu_available, name, snr, count, T, cn, schedule):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = _ref(name, snr, count, T, cn, schedule)
    if not name.startswith("BCH"):  # both exits are exercised
        assert (want["status"] == 0).sum() >= 3 and (want["status"] != 0).sum() >= 3
    g = _graph(name)
    assert phys_kernel_name(g, cn=cn, schedule=schedule) == \
        ("phys_layered_kernel" if schedule == "layered" else phys_kernel_name(g))
    got = phys_decode(g, _frames(name, snr, count), T, post=True, cn=cn, schedule=schedule, alpha=ALPHA, beta=BETA)
    _assert_equal(got, want, f"{name} {cn} {schedule}")


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["flooding", "layered"])
def test_one_iteration_and_single_frame(gpu_available, schedule):
    from ldpc_amd.device import phys_decode
    name, snr = "wimax_576_0.5", -2.5
    g, llr = _graph(name), _frames(name, snr, 96)
    got = phys_decode(g, llr, 1, post=True, cn="nms", schedule=schedule, alpha=ALPHA)
    _assert_equal(got, _ref(name, snr, 96, 1, "nms", schedule), f"T=1 {schedule}")
    got = phys_decode(g, llr[:1], 20, post=True, cn="oms", schedule=schedule, beta=BETA)
    _assert_equal(got, _ref(name, snr, 96, 20, "oms", schedule, first=1), f"one frame {schedule}")


@pytest.mark.gpu
@pytest.mark.parametrize("cn", ["nms", "oms"])
def test_hbm_path_bit_identical_to_lds(gpu_available, cn):
    """96 frames: one full 64-frame tile and one half tile."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    name, snr = "wimax_576_0.5", -2.5
    g, llr = _graph(name), _frames(name, snr, 96)
    assert phys_kernel_name(g, hbm=True, cn=cn) == "phys_cn_tile_kernel"
    a = phys_decode(g, llr, 20, post=True, cn=cn, alpha=ALPHA, beta=BETA)
    b = phys_decode(g, llr, 20, post=True, cn=cn, alpha=ALPHA, beta=BETA, hbm=True)
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(a.post.view(np.uint32), b.post.view(np.uint32))
    _assert_equal(b, _ref(name, snr, 96, 20, cn, "flooding"), f"hbm {cn}")


@pytest.mark.gpu
def test_unsupported_combinations(gpu_available):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    name = "wimax_576_0.5"
    g, llr = _graph(name), _frames(name, -2.5, 96)[:4]
    with pytest.raises(ldpc_amd.LdpcError) as e:
        phys_decode(g, llr, 5, cn="nms", schedule="layered", hbm=True)
    assert e.value.code == _lib.LDPC_ERANGE and "layered" in str(e.value)
    assert phys_kernel_name(g, hbm=True, cn="nms", schedule="layered") == ""
    # sum-product layered: the Python layer refuses it, and so does the library
    z = np.empty((4, g.n), np.uint8)
    rc = _lib.gpu().ldpc_phys_decode_ex(g.handle, 4, _lib.ptr(np.ascontiguousarray(llr)), 5, 0, _lib.LDPC_CN_SPA,
                                        _lib.LDPC_SCHED_LAYERED, 0.0, _lib.ptr(z), None, None, None, None, None)
    assert rc == _lib.LDPC_EINVAL and b"layered" in _lib.lib().ldpc_last_error()
    with pytest.raises(ldpc_amd.LdpcError) as e:
        _lib.check("ldpc_phys_decode_ex", rc)
    assert e.value.code == _lib.LDPC_EINVAL
    # the library's own parameter checks (the Python layer never lets these through)
    for rule, sched, param in ((_lib.LDPC_CN_NMS, 0, 0.0), (_lib.LDPC_CN_NMS, 0, 1.5), (_lib.LDPC_CN_OMS, 0, -1.0),
                               (3, 0, 0.5), (_lib.LDPC_CN_NMS, 2, 0.5)):
        rc = _lib.gpu().ldpc_phys_decode_ex(g.handle, 4, _lib.ptr(np.ascontiguousarray(llr)), 5, 0, rule, sched,
                                            param, _lib.ptr(z), None, None, None, None, None)
        assert rc == _lib.LDPC_EINVAL, (rule, sched, param)


@pytest.mark.gpu
def test_default_options_through_ex_entry_equal_old_entry(gpu_available):
    from ldpc_amd.device import phys_decode
    name = "wimax_576_0.5"
    g, llr = _graph(name), _frames(name, -2.5, 96)
    old = phys_decode(g, llr, 20, post=True)  # ldpc_phys_decode
    new = phys_decode(g, llr, 20, post=True, cn="spa", schedule="flooding", ex=True)  # ldpc_phys_decode_ex
    assert 0 < (old.status == 0).sum() < 96
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(old[key], new[key], err_msg=key)
    np.testing.assert_array_equal(old.post.view(np.uint32), new.post.view(np.uint32))


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
        got = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", schedule=schedule, alpha=ALPHA)
        for p, (u, llr) in enumerate(frames):
            o = minsum_ref.decode(Hp, llr, T, "nms", schedule, ALPHA, BETA)
            w = oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])
            want[schedule, p] = w
            np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w[[0, 1, 2, 3, 4, 6]],
                                          err_msg=f"{schedule} point {p}")
    assert 0 < want["layered", 0][1] < B and want["layered", 1][1] == 0  # waterfall, then error-free
    res, ctr = mc.simulate(name, list(snrs), B, T, seed=SEED, mode="physical", cn_rule="nms", schedule="layered",
                           alpha=ALPHA)
    assert res.config.decoder_type == "minsum-normalized-layered"
    for p, sp in enumerate(res.snr_points):
        w = want["layered", p]
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w[[0, 1, 2, 3, 4, 6]])
        assert (sp.total_blocks, sp.failed_blocks) == (B, int(w[1]))
        assert sp.fer == w[1] / B and sp.ber == w[2] / (edd._k * B)
