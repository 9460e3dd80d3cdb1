"""Host side of physical mode's fixed-point min-sum decoder: the contract's two
worked values through the numpy restatement (tests/qminsum_ref.py), the
argument checks of the Python and command-line interfaces, decoder_type and
the four new C entries.  No GPU."""
import os
import re

import numpy as np
import pytest

import ldpc_amd
import oracle
import qminsum_ref
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from conftest import ROOT

SEED = 20260213
NEW_SYMBOLS = ("ldpc_phys_decode_q", "ldpc_phys_mc_run_q", "ldpc_phys_kernel_name_q", "ldpc_phys_q_lds_bytes")


def test_worked_check_row():
    """q = 6, NMS alpha_q = 12, L - E = [5, -3, 40, 0]."""
    qmax, pmax = qminsum_ref.limits(6)
    assert (qmax, pmax) == (31, 127) and qminsum_ref.limits(8) == (127, 511) and qminsum_ref.limits(4) == (7, 31)
    Q = np.clip(np.array([[5, -3, 40, 0]], np.int32), -qmax, qmax)
    np.testing.assert_array_equal(Q, [[5, -3, 31, 0]])
    np.testing.assert_array_equal(qminsum_ref.check(Q, "nms", 12), [[0, 0, 0, -2]])
    # offset rule on the same row: magnitudes max([0, 0, 0, 3] - 2, 0)
    np.testing.assert_array_equal(qminsum_ref.check(Q, "oms", 2), [[0, 0, 0, -1]])
    # a tie: min2 == min1, every edge gets it
    np.testing.assert_array_equal(qminsum_ref.check(np.array([[4, -4, 9]], np.int32), "nms", 16), [[-4, 4, -4]])


def test_worked_load_ties_round_to_even():
    np.testing.assert_array_equal(qminsum_ref.quantize([[0.625, 0.875, -0.625, -0.875]], 6, 4.0), [[-2, -4, 2, 4]])
    # the clamp: +-Qmax, in float before the conversion
    np.testing.assert_array_equal(qminsum_ref.quantize([[100.0, -100.0, 7.75, 1e30]], 6, 4.0), [[-31, 31, -31, -31]])
    np.testing.assert_array_equal(qminsum_ref.quantize([[1.0, -2.0]], 4, 1.0), [[-1, 2]])


def test_restatement_decodes_and_layered_has_no_posterior_clamp():
    edd = ldpc_amd.load_committed_code("wimax_576_0.5")
    _, c, llr = oracle.generate_frames(edd._h_std, SEED, 2, mc.sigma_for_snr(-2.0), 0, 48)
    Hp = edd.physical_matrix()
    for schedule in ("flooding", "layered"):
        r = qminsum_ref.decode(Hp, llr, 20, "nms", schedule, 6, 4.0, 12)
        ok = r["status"] == 0
        assert ok.mean() >= 0.5 and r["post"].dtype == np.int16
        np.testing.assert_array_equal((r["z"] ^ 1)[ok], c[ok])  # converged frames are the sent codewords
        np.testing.assert_array_equal(r["iters"], np.where(ok, r["conv"] + 1, 20))
        assert np.abs(r["post"]).max() <= (127 if schedule == "flooding" else 62)
        if schedule == "layered":
            assert r["counts"]["post_clamps"] == 0


BAD = [dict(qbits=3), dict(qbits=9), dict(qbits=6.5), dict(llr_scale=0.0), dict(llr_scale=-1.0),
       dict(llr_scale=float("inf")), dict(llr_scale=float("nan")),
       dict(alpha=0.03),            # alpha_q = round(0.48) = 0
       dict(cn="oms", beta=8.0),    # beta_q = 32 > Qmax = 31 at q = 6, scale 4
       dict(cn="oms", qbits=4, llr_scale=1.0, beta=8.0),  # beta_q = 8 > Qmax = 7
       dict(cn="spa")]


@pytest.mark.parametrize("kw", BAD)
def test_python_argument_validation(kw):
    from ldpc_amd import device
    kw = {"cn": "nms", "qbits": 6, **kw}
    with pytest.raises(ValueError):
        device.phys_decode(None, np.zeros((1, 7)), 5, **kw)  # before it touches the graph or a device
    with pytest.raises(ValueError):
        device.Decoder.phys_mc_run(None, None, SEED, [1.0], 1, 0, 5, **kw)
    if not {"alpha", "beta"} & set(kw):  # the kernel's name does not depend on them
        with pytest.raises(ValueError):
            device.phys_kernel_name(None, **kw)
    sim = {("cn_rule" if k == "cn" else k): v for k, v in kw.items()}
    with pytest.raises(ValueError):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, mode="physical", **sim)


def test_alpha_q_17_is_unreachable_through_alpha_but_rejected():
    """alpha <= 1 is phys_rule_args' own bound, so alpha_q = 17 needs alpha > 1:
    both checks say ValueError."""
    from ldpc_amd import device
    with pytest.raises(ValueError):
        device.phys_quant_args("nms", alpha=1.05, qbits=6)  # round(16.8) = 17
    with pytest.raises(ValueError):
        device.phys_decode(None, np.zeros((1, 7)), 5, cn="nms", alpha=1.05, qbits=6)


def test_python_arguments_accepted():
    from ldpc_amd import device
    assert device.phys_quant_args("nms", alpha=0.75, qbits=6) == (6, 4.0, 12)
    assert device.phys_quant_args("nms", alpha=1.0, qbits=4, llr_scale=1) == (4, 1.0, 16)
    assert device.phys_quant_args("nms", alpha=0.04, qbits=8, llr_scale=8) == (8, 8.0, 1)
    assert device.phys_quant_args("oms", beta=0.5, qbits=6, llr_scale=4.0) == (6, 4.0, 2)
    assert device.phys_quant_args("oms", beta=0.0, qbits=5, llr_scale=2.0) == (5, 2.0, 0)
    assert device.phys_quant_args("oms", beta=7.75, qbits=6, llr_scale=4.0) == (6, 4.0, 31)
    with pytest.raises(ValueError):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, cn_rule="spa", qbits=6)  # needs mode="physical"


def test_decoder_type():
    assert mc.decoder_type("nms", "layered", 6) == "minsum-normalized-layered-q6"
    assert mc.decoder_type("oms", "flooding", qbits=8) == "minsum-offset-q8"
    assert mc.decoder_type("nms", "layered") == "minsum-normalized-layered"
    assert mc.decoder_type() == "sumproduct"


def test_cli_options(capsys):
    a = mc.parse_args(["--matrix", "wimax_576_0.5"])
    assert (a.qbits, a.llr_scale) == (None, 4.0)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered",
                       "--qbits", "6", "--llr-scale", "4"])
    assert (a.mode, a.cn_rule, a.schedule, a.qbits, a.llr_scale) == ("physical", "nms", "layered", 6, 4.0)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--cn-rule", "oms", "--qbits", "5", "--llr-scale", "2.5"])
    assert (a.cn_rule, a.qbits, a.llr_scale) == ("oms", 5, 2.5)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--cn-rule", "nms", "--qbits", "8"])
    assert (a.qbits, a.llr_scale) == (8, 4.0)
    for argv in (["--qbits", "6"], ["--llr-scale", "4"],                      # need --mode physical
                 ["--cn-rule", "nms", "--qbits", "6"],
                 ["--mode", "physical", "--qbits", "6"],                      # sum-product (the default rule)
                 ["--mode", "physical", "--cn-rule", "spa", "--qbits", "6"],
                 ["--mode", "physical", "--cn-rule", "nms", "--qbits", "3"],
                 ["--mode", "physical", "--cn-rule", "nms", "--qbits", "9"],
                 ["--mode", "physical", "--cn-rule", "nms", "--qbits", "6", "--llr-scale", "0"],
                 ["--mode", "physical", "--cn-rule", "nms", "--llr-scale", "4"],   # no --qbits
                 ["--mode", "physical", "--cn-rule", "oms", "--qbits", "6", "--beta", "9"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(["--matrix", "x"] + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_new_symbols_exported_and_declared():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ldpc_hip.h")).read(), flags=re.S)
    L = _lib.lib()
    for sym in NEW_SYMBOLS:
        assert sym in _lib.EXPORTED, sym
        assert re.search(rf"\b{sym}\s*\(", txt), f"{sym} not declared in the header"
        assert hasattr(L, sym), sym
    assert L.ldpc_abi_version() == 5


def test_q_entries_reject_null_graph_without_touching_gpu():
    L = _lib.lib()
    assert L.ldpc_phys_decode_q(None, 1, None, 5, 0, 1, 0, 6, 4.0, 12, None, None, None, None, None, None) == -22
    assert b"ldpc_phys_decode_q" in L.ldpc_last_error()
    assert L.ldpc_phys_mc_run_q(None, None, 1, 1, None, 1, 0, 5, 0, 1, 0, 6, 4.0, 12, None, None) == -22
    assert b"ldpc_phys_mc_run_q" in L.ldpc_last_error()
    assert L.ldpc_phys_kernel_name_q(None, 0, 1, 0, 6) == b""
    assert L.ldpc_phys_q_lds_bytes(None, 0) == -1
