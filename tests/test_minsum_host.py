"""Host side of physical mode's min-sum rules and layered schedule: the layer
builder (ldpc_layers_build / ldpc_amd.build_layers) against the numpy
first-fit, the restatement's own sanity, and the argument checks of the Python
and command-line interfaces.  No GPU."""
import ctypes

import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import oracle
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc

SEED = 20260213
# code -> (layers, smallest layer, largest layer, max row degree, max column degree)
LAYERS = {
    "BCH_7_4_1_strip": (3, 1, 1, 4, 3),
    "wimax_576_0.5": (7, 24, 48, 7, 6),
    "wimax_2304_0.5": (7, 96, 192, 7, 6),
    "wimax_2304_0.75A": (6, 96, 96, 15, 4),
    "wimax_2304_0.75B": (6, 96, 96, 15, 6),
}


@pytest.mark.parametrize("name", sorted(LAYERS))
def test_layers_equal_numpy_first_fit(name):
    Hp = ldpc_amd.load_committed_code(name).physical_matrix()
    lp, lr = ldpc_amd.build_layers(Hp)
    assert lp.dtype == np.int32 and lr.dtype == np.int32
    rp, rr = minsum_ref.first_fit_layers(Hp)
    np.testing.assert_array_equal(lp, rp)
    np.testing.assert_array_equal(lr, rr)
    nl, lo, hi, rdeg, cdeg = LAYERS[name]
    sizes = np.diff(lp)
    assert (len(sizes), sizes.min(), sizes.max()) == (nl, lo, hi)
    assert np.diff(Hp.indptr).max() == rdeg and np.diff(Hp.tocsc().indptr).max() == cdeg
    # every row exactly once; rows ascending and column-disjoint inside a layer
    np.testing.assert_array_equal(np.sort(lr), np.arange(Hp.shape[0]))
    for l in range(nl):
        rows = lr[lp[l]:lp[l + 1]]
        assert (np.diff(rows) > 0).all()
        assert Hp[rows].sum(axis=0).max() == 1


def _layers_rc(m, n, indptr, indices):
    indptr, indices = _lib.as_i32(indptr), _lib.as_i32(indices)
    out = np.zeros(max(m, 1), np.int32)
    nl = ctypes.c_int32(-1)
    return _lib.lib().ldpc_layers_build(m, n, _lib.i32p(indptr), _lib.i32p(indices), _lib.i32p(out),
                                        ctypes.byref(nl)), out, nl.value


def test_layers_build_small_and_malformed():
    # rows 0 and 2 share no column, row 1 clashes with both
    rc, out, nl = _layers_rc(3, 6, [0, 2, 4, 6], [0, 1, 1, 2, 2, 3])
    assert (rc, nl, out.tolist()) == (0, 2, [0, 1, 0])
    bad = [
        (3, 6, [1, 2, 4, 6], [0, 1, 1, 2, 2, 3]),   # row_ptr[0] != 0
        (3, 6, [0, 4, 2, 6], [0, 1, 1, 2, 2, 3]),   # row_ptr not monotone
        (3, 6, [0, 2, 4, 6], [0, 1, 1, 6, 2, 3]),   # column out of range
        (3, 6, [0, 2, 4, 6], [1, 0, 1, 2, 2, 3]),   # row not ascending
        (3, 6, [0, 2, 4, 6], [0, 0, 1, 2, 2, 3]),   # duplicate entry
        (3, 2, [0, 2, 4, 6], [0, 1, 0, 1, 0, 1]),   # m > n
    ]
    for m, n, rp, ci in bad:
        assert _layers_rc(m, n, rp, ci)[0] == _lib.LDPC_EINVAL, (rp, ci)
    L = _lib.lib()
    assert L.ldpc_layers_build(3, 6, None, None, None, None) == _lib.LDPC_EINVAL
    assert b"ldpc_layers_build" in L.ldpc_last_error()
    with pytest.raises(ldpc_amd.LdpcError):
        ldpc_amd.build_layers(np.array([[1, 1, 0], [0, 1, 1], [1, 0, 1], [1, 1, 1]]))  # m > n


def test_restatement_layered_converges_faster():
    """wimax_576_0.5 at -2.0 dB: layering lowers the iteration count, both decode."""
    edd = ldpc_amd.load_committed_code("wimax_576_0.5")
    _, c, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(-2.0), 0, 96)
    Hp = edd.physical_matrix()
    fl = minsum_ref.decode(Hp, llr, 20, "nms", "flooding")
    la = minsum_ref.decode(Hp, llr, 20, "nms", "layered")
    assert la["iters"].mean() < fl["iters"].mean(), (la["iters"].mean(), fl["iters"].mean())
    for r in (fl, la):
        assert r["status"].mean() <= 0.10
        ok = r["status"] == 0
        np.testing.assert_array_equal((r["z"] ^ 1)[ok], c[ok])  # converged frames are the sent codewords
        np.testing.assert_array_equal(r["iters"], np.where(ok, r["conv"] + 1, 20))


def test_restatement_rejects_degree_one_row():
    with pytest.raises(ValueError):
        minsum_ref.decode(np.array([[1, 1, 0], [0, 0, 1]]), np.zeros((1, 3)), 2)


@pytest.mark.parametrize("kw", [dict(cn="min"), dict(schedule="serial"), dict(cn="nms", alpha=0.0),
                                dict(cn="nms", alpha=1.5), dict(cn="nms", alpha=float("nan")),
                                dict(cn="oms", beta=-0.1), dict(cn="spa", schedule="layered")])
def test_python_argument_validation(kw):
    from ldpc_amd import device
    with pytest.raises(ValueError):
        device.phys_rule_args(**kw)
    # phys_decode / phys_mc_run / simulate check before they touch the graph or a device
    with pytest.raises(ValueError):
        device.phys_decode(None, np.zeros((1, 7)), 5, **kw)
    with pytest.raises(ValueError):
        device.Decoder.phys_mc_run(None, None, SEED, [1.0], 1, 0, 5, **kw)
    sim = {("cn_rule" if k == "cn" else k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, mode="physical", **sim)


def test_python_arguments_accepted():
    from ldpc_amd import device
    assert device.phys_rule_args() == (0, 0, 0.0)
    assert device.phys_rule_args("nms", "layered", alpha=1.0) == (1, 1, 1.0)
    assert device.phys_rule_args("oms", "flooding", beta=0.0) == (2, 0, 0.0)
    with pytest.raises(ValueError):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, cn_rule="nms")  # needs mode="physical"
    assert mc.decoder_type() == "sumproduct"
    assert mc.decoder_type("nms", "layered") == "minsum-normalized-layered"
    assert mc.decoder_type("oms") == "minsum-offset"


def test_cli_options(capsys):
    a = mc.parse_args(["--matrix", "wimax_576_0.5"])
    assert (a.mode, a.cn_rule, a.schedule, a.alpha, a.beta) == ("parity", "spa", "flooding", 0.75, 0.5)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered",
                       "--alpha", "0.8"])
    assert (a.mode, a.cn_rule, a.schedule, a.alpha, a.beta) == ("physical", "nms", "layered", 0.8, 0.5)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--cn-rule", "oms", "--beta", "0.25"])
    assert (a.cn_rule, a.schedule, a.beta) == ("oms", "flooding", 0.25)
    for argv in (["--cn-rule", "nms"], ["--schedule", "layered"], ["--alpha", "0.8"], ["--beta", "0.5"],
                 ["--mode", "physical", "--schedule", "layered"],  # sum-product layered
                 ["--mode", "physical", "--cn-rule", "nms", "--alpha", "2"],
                 ["--mode", "physical", "--cn-rule", "ams"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(["--matrix", "x"] + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_decode_ex_rejects_null_graph_without_touching_gpu():
    L = _lib.lib()
    assert L.ldpc_phys_decode_ex(None, 1, None, 5, 0, 1, 1, 0.75, None, None, None, None, None, None) == -22
    assert b"ldpc_phys_decode_ex" in L.ldpc_last_error()
    assert L.ldpc_phys_mc_run_ex(None, None, 1, 1, None, 1, 0, 5, 0, 1, 1, 0.75, None, None) == -22
    assert L.ldpc_phys_kernel_name_ex(None, 0, 1, 1) == b""
    assert (_lib.LDPC_CN_SPA, _lib.LDPC_CN_NMS, _lib.LDPC_CN_OMS) == (0, 1, 2)
    assert (_lib.LDPC_SCHED_FLOODING, _lib.LDPC_SCHED_LAYERED) == (0, 1)
