"""Host side of the physical-mode rate matching (ldpc_rate_match_set /
ldpc_rate_match_get, ldpc_amd.ratematch): the pattern's validation, the command
line's column grammar, the effective rate and the Eb/N0 axis, simulate()'s
refusals, the argument checks that need no device, the header, the stats-json
document, the library's host logic as a stand-alone program, and the numpy
restatement's own encoder (tests/ratematch_ref.py).  No GPU."""
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, hstd_for
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0, sigmas_for_axis
from ldpc_amd.ratematch import KNOWN_LLR, RateMatch, parse_columns

NEW = ("ldpc_rate_match_set", "ldpc_rate_match_get")
W576 = RateMatch(tuple(288 + 6 * i for i in range(48)), tuple(range(24)))


def test_rate_match_validation_table():
    assert RateMatch() == RateMatch((), ()) and RateMatch().is_empty
    assert RateMatch([9, 3], [1]).punctured == (3, 9)  # kept ascending
    RateMatch().validate(7, 4, 2)  # an empty pattern asks nothing of E
    W576.validate(576, 288)
    for bps in (1, 2, 4, 6):
        W576.validate(576, 288, bps)
    ok = RateMatch((0, 7, 45, 46, 47, 65), (1, 33, 44))
    assert ok.validate(66, 46, 1) is ok
    for rm, n, k, bps, msg in ((RateMatch((66,)), 66, 46, None, "outside"),
                               (RateMatch((-1,)), 66, 46, None, "outside"),
                               (RateMatch((), (-2,)), 66, 46, None, "outside"),
                               (RateMatch((5,), (5,)), 66, 46, None, "twice"),
                               (RateMatch((5, 5)), 66, 46, None, "twice"),
                               (RateMatch((), (46,)), 66, 46, None, "information column"),
                               (RateMatch(tuple(range(21, 66)), tuple(range(21))), 66, 46, None, "E < 1"),
                               (RateMatch((), tuple(range(46))), 66, 46, None, "information bit"),
                               (ok, 66, 46, 2, "E = 57.*bps = 2"),
                               (ok, 66, 46, 6, "E = 57.*bps = 6")):
        with pytest.raises(ValueError, match=msg):
            rm.validate(n, k, bps)
    for bad in ("0:4", (1.5,), ("a",), 7):
        with pytest.raises((ValueError, TypeError)):
            RateMatch(bad)
    with pytest.raises(Exception):
        W576.punctured = ()  # frozen


def test_transmitted_and_effective_rate_hand_values():
    assert RateMatch((0, 3), (1,)).transmitted(6) == [2, 4, 5]
    assert RateMatch().transmitted(4) == [0, 1, 2, 3] and RateMatch().effective_rate(576, 288) == 0.5
    assert W576.n_transmitted(576) == 504 and W576.info_bits(288) == 264
    assert W576.effective_rate(576, 288) == 264 / 504
    # wimax_2304_0.5 with a sixth of its parity bits punctured: 1152 / 2112 = 6/11
    rm = RateMatch(parse_columns("k:n:6", 2304, 1152))
    assert len(rm.punctured) == 192 and rm.effective_rate(2304, 1152) == pytest.approx(6 / 11, rel=1e-15)
    # the Eb/N0 axis at the effective rate: Es = rate bps Eb
    assert sigma_for_ebn0(4.0, 264 / 504, 4) == pytest.approx(
        math.sqrt(1.0 / (2 * (264 / 504) * 4 * 10 ** 0.4)), rel=1e-15)
    assert sigmas_for_axis(ChannelSpec("awgn", "qam16"), "ebn0", [4.0], W576.effective_rate(576, 288)) == \
        [sigma_for_ebn0(4.0, 264 / 504, 4)]
    # puncturing raises the rate, so the same Eb/N0 is less noise per symbol; shortening lowers it
    assert sigma_for_ebn0(4.0, 6 / 11, 1) < sigma_for_ebn0(4.0, 0.5, 1) < sigma_for_ebn0(4.0, 264 / 552, 1)
    assert W576.info(576, 288) == {"punctured": list(W576.punctured), "shortened": list(range(24)),
                                   "transmitted": 504, "info_bits": 264, "rate": 264 / 504}
    assert KNOWN_LLR == 1.0e4


def test_parse_columns_accept_reject_table():
    n, k = 576, 288
    assert parse_columns("k:n:6", n, k) == W576.punctured
    assert parse_columns("0:24", n, k) == tuple(range(24))
    assert parse_columns("n-48:n", n, k) == tuple(range(528, 576))
    assert parse_columns("5", n, k) == (5,) and parse_columns("k", n, k) == (288,)
    assert parse_columns("k-1, 0:2 ,n-1", n, k) == (0, 1, 287, 575)
    assert parse_columns("k+4:k+20:5", n, k) == (292, 297, 302, 307)
    assert parse_columns("k - 2 : k + 2", n, k) == (286, 287, 288, 289)
    assert parse_columns("10:10", n, k) == ()  # an empty slice, as Python's
    assert parse_columns("0:n", 8, 4) == tuple(range(8))
    for bad in ("", " ", ",", "1,,2", "a", "k*2", "m", "1:2:3:4", "1:", ":4", "0:8:0", "0:8:-1", "0:8:x", "n", "0:n+1",
                "n:n+2", "-1", "-3:4", "k-300:4", "1.5", "3,3", "0:4,2", "k+", "kn"):
        with pytest.raises(ValueError):
            parse_columns(bad, n, k)
    with pytest.raises(ValueError):
        parse_columns(None, n, k)


def test_cli_accept_reject_table(capsys):
    head = ["--matrix", "wimax_576_0.5"]
    phys = ["--mode", "physical", "--cn-rule", "nms", "--schedule", "layered"]
    a = mc.parse_args(head)
    assert a.puncture is None and a.shorten is None and mc.cli_rate_match(a) is None
    a = mc.parse_args(head + phys + ["--channel", "awgn", "--modulation", "qam16", "--puncture", "k:n:6",
                                     "--shorten", "0:24"])
    assert mc.cli_rate_match(a) == W576
    a = mc.parse_args(head + phys + ["--channel", "rayleigh", "--shorten", "0:24"])
    assert mc.cli_rate_match(a) == RateMatch((), tuple(range(24)))
    a = mc.parse_args(["--matrix", "ira_1440_0.5"] + phys + ["--channel", "awgn", "--puncture", "k+4:n:5"])
    assert mc.code_shape("ira_1440_0.5") == (1440, 720)
    assert mc.cli_rate_match(a).punctured == tuple(724 + 5 * i for i in range(144))
    for argv in (["--puncture", "k:n:6"],                                  # no --mode physical
                 ["--mode", "parity", "--shorten", "0:24"],
                 phys + ["--puncture", "k:n:6"],                           # the reference channel
                 phys + ["--channel", "reference", "--shorten", "0:24"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    model = phys + ["--channel", "awgn", "--modulation", "qam16"]
    for argv, msg in ((["--shorten", "k:k+2"], "information column"),
                      (["--puncture", "0:3"], "E = 573.*bps = 4"),
                      (["--puncture", "0:n"], "E < 1"),
                      (["--puncture", "0:4", "--shorten", "3:5"], "twice"),
                      (["--puncture", "k:n:0"], "step"),
                      (["--puncture", "n:n+4"], "outside")):
        with pytest.raises(ValueError, match=msg):
            mc.cli_rate_match(mc.parse_args(head + model + argv))


def test_cli_refuses_before_any_device_call(monkeypatch, capsys):
    """main() turns a bad pattern into an exit before simulate() is reached."""
    def no_simulate(*a, **k):
        raise AssertionError("main() reached simulate() with a pattern it should have refused")
    monkeypatch.setattr(mc, "simulate", no_simulate)
    with pytest.raises(SystemExit, match="information column"):
        mc.main(["--matrix", "wimax_576_0.5", "--mode", "physical", "--channel", "awgn", "--shorten", "k:k+2"])


def test_simulate_refuses_before_any_device_call(monkeypatch):
    """matrix=None: simulate() raises before it loads a code or makes a graph."""
    qam = ChannelSpec("awgn", "qam16")
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, rate_match=W576)
    with pytest.raises(ValueError, match="channel model"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", rate_match=W576)
    with pytest.raises(ValueError, match="channel model"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel=ChannelSpec(), rate_match=W576)
    with pytest.raises(ValueError, match="RateMatch"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel=qam, rate_match=((1,), ()))
    # once the code is known: before a graph is made
    from ldpc_amd import device

    def no_graph(*a, **k):
        raise AssertionError("simulate() made a graph before it checked the pattern")
    monkeypatch.setattr(device, "Graph", no_graph)
    with pytest.raises(ValueError, match="information column"):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, mode="physical", channel=qam, rate_match=RateMatch((), (288,)))
    with pytest.raises(ValueError, match="E = 573.*bps = 4"):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, mode="physical", channel=qam, rate_match=RateMatch((0, 1, 2)))
    with pytest.raises(ValueError, match="E = 1437.*bps = 2"):
        mc.simulate("ira_1440_0.5", [0.0], 1, 5, mode="physical", cn_rule="nms", channel=ChannelSpec("awgn", "qpsk"),
                    rate_match=RateMatch((0, 1, 2)))
    # BCH n = 7 under QPSK: the pattern's E = 6 replaces the n % bps check
    with pytest.raises(AssertionError, match="made a graph"):
        mc.simulate("BCH_7_4_1_strip", [0.0], 1, 5, mode="physical", channel=ChannelSpec("awgn", "qpsk"),
                    rate_match=RateMatch((6,)))
    assert mc.rate_match_shape(None, qam, 576, 288) == (576, 288, 0.5)
    assert mc.rate_match_shape(W576, qam, 576, 288) == (504, 264, 264 / 504)


def test_point_results_take_the_information_bits():
    ctr = np.array([[200, 50, 1320, 300, 150, 0, 0]], np.int64)
    assert mc.point_results(ctr, 264, [4.0])[0].ber == 1320 / (264 * 200)


def test_stats_json_rate_match_object(tmp_path):
    spec = ChannelSpec("awgn", "qam16", "maxlog")
    rate = W576.effective_rate(576, 288)
    info = mc.channel_info(spec, None, [4.0, 8.0], rate, W576, 576, 288)
    assert info["sigma"] == [sigma_for_ebn0(4.0, 264 / 504, 4), sigma_for_ebn0(8.0, 264 / 504, 4)]
    assert info["rate_match"] == {"punctured": list(W576.punctured), "shortened": list(range(24)), "transmitted": 504,
                                  "info_bits": 264, "rate": 264 / 504}
    assert "rate_match" not in mc.channel_info(spec, None, [4.0], 0.5)
    assert "rate_match" not in mc.channel_info(spec, None, [4.0], 0.5, RateMatch(), 576, 288)
    st = mc.reduce_stats([{"hist": np.array([0, 3, 1]), "undetected_frames": 0, "undetected_bit_errors": 0,
                           "failed": np.zeros((0, 2), np.int64), "failed_dropped": 1}], [4.0])
    path = tmp_path / "s.json"
    mc.stats_to_json(str(path), 7, st, channel=info)
    doc = json.loads(path.read_text())
    assert doc["channel"]["rate_match"]["transmitted"] == 504 and doc["channel"]["rate_match"]["info_bits"] == 264
    assert doc["channel"]["rate_match"]["rate"] == 264 / 504 and doc["channel"]["rate_match"]["punctured"][:2] == [288, 294]
    head = mc.rate_match_header(info["rate_match"], 576, 288)
    assert "E 504" in head and "punctured 48" in head and "shortened 24" in head and "0.523810" in head


def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert re.search(r"^#define\s+LDPC_RM_KNOWN_LLR\s+1\.0e4\b", txt, flags=re.M)
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5


_NULL_CALLS = r"""
import ctypes, os
from ldpc_amd import _lib
L = _lib.lib()
cols = (ctypes.c_int32 * 3)(1, 2, 3)
n, s = ctypes.c_int32(), ctypes.c_int32()
calls = [("NULL decoder", lambda: L.ldpc_rate_match_set(None, 3, cols, 0, None), b"NULL decoder"),
         ("NULL decoder, clearing", lambda: L.ldpc_rate_match_set(None, 0, None, 0, None), b"NULL decoder"),
         ("NULL decoder, bad counts", lambda: L.ldpc_rate_match_set(None, -1, None, 0, None), b"NULL decoder"),
         ("get NULL", lambda: L.ldpc_rate_match_get(None, ctypes.byref(n), ctypes.byref(s), None, 0, None, 0),
          b"NULL decoder")]
for what, call, msg in calls:
    rc = call()
    assert rc == _lib.LDPC_EINVAL, (what, rc)
    assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
assert not _lib.hip_started_here()
# no device node was opened: the runtime was never started
opened = [os.readlink(f"/proc/self/fd/{fd}") for fd in os.listdir("/proc/self/fd")
          if os.path.exists(f"/proc/self/fd/{fd}")]
assert not [p for p in opened if p.startswith("/dev/kfd") or p.startswith("/dev/dri")], opened
print("ok")
"""


def test_rate_match_set_argument_checks_touch_no_device():
    """In a process of its own: nothing else in it can have started the runtime."""
    env = dict(os.environ, PYTHONPATH=PKG_DIR + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NULL_CALLS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_library_host_logic_stand_alone(tmp_path):
    """csrc/rate_match_host.h (what ldpc_rate_match_set validates with and the
    tables the kernels read) in tools/rate_match_host_check.cpp, a program of
    its own."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "rate_match_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(PKG_DIR, "csrc"),
                    os.path.join(ROOT, "tools", "rate_match_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "rate_match_host_check: OK" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------ the restatement's self-checks
def test_restatement_encoder_and_scatter():
    import oracle
    import ratematch_ref
    from ldpc_amd import ira
    from scipy import sparse
    seed = 20260213
    for H, is_ira, rm in ((hstd_for("wimax_576_0.5"), False, W576),
                          (sparse.csr_matrix(ira.small_ira_matrix()), True,
                           RateMatch(tuple(724 + 5 * i for i in range(144)), tuple(range(672, 720))))):
        # without a pattern the re-encoder gives the committed frame source's codewords
        u0, c0, _ = oracle.generate_frames(H, seed, 3, 1.0, 1000, 3, ira=is_ira)
        np.testing.assert_array_equal(ratematch_ref.encode(H, u0, is_ira), c0)
        u, c = ratematch_ref.bits(H, is_ira, rm, seed, 3, 1000, 3)
        sh = list(rm.shortened)
        assert not u[:, sh].any() and u0[:, sh].any()
        keep = np.setdiff1d(np.arange(u.shape[1]), sh)
        np.testing.assert_array_equal(u[:, keep], u0[:, keep])
        assert (c != c0)[:, u.shape[1]:].any()  # shortening changed parities
        spec = ChannelSpec("awgn", "qam16", "maxlog")
        llr, M = ratematch_ref.frames_llr(spec, rm, c, seed, 3, 0.3, 1000)
        n = c.shape[1]
        assert (llr[:, list(rm.punctured)] == 0.0).all() and (llr[:, sh] == -1.0e4).all()
        tx = rm.transmitted(n)
        assert np.isfinite(llr).all() and (np.abs(llr[:, tx]) > 0).all() and (M > 0).all()
        # at a vanishing sigma the transmitted columns carry the codeword's signs
        quiet, _ = ratematch_ref.frames_llr(spec, rm, c, seed, 3, 1e-4, 1000)
        np.testing.assert_array_equal(quiet[:, tx] > 0, c[:, tx] == 1)
