"""Constellation tables of the physical-mode frame source, everything that
needs no GPU: the Python builders and their validation, the library's
argument checks (no device is touched), the command line's accept / reject
table, the Eb/N0 axis, and the numpy restatement's self-checks
(tests/constellation_ref.py): against tests/channel_ref.py on a table that
spells out 16-QAM, and the error rates of the two built-in labellings.
"""
import cmath
import json
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import channel_ref
import constellation_ref
from conftest import PKG_DIR, ROOT
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0, sigma_for_esn0, sigmas_for_axis
from ldpc_amd.constellation import Constellation, effective_bps, parse

NEW = ("ldpc_constellation_set", "ldpc_constellation_get")


def _energy(c):
    return sum(abs(p) ** 2 for p in c.points) / len(c.points)


# ---------------------------------------------------------------- builders
def test_builders_have_unit_energy_and_the_stated_shape():
    p8, a16 = Constellation.psk8(), Constellation.apsk16()
    assert (p8.name, p8.bps, len(p8.points)) == ("8psk", 3, 8)
    assert (a16.name, a16.bps, len(a16.points)) == ("16apsk", 4, 16)
    for c in (p8, a16, Constellation.apsk16(2.57)):
        assert abs(_energy(c) - 1.0) <= 1e-12, c.name
    assert Constellation.apsk16(2.57).name == "16apsk:2.57"
    # the builders are the restatement's written-out tables
    np.testing.assert_allclose(np.array(p8.points), constellation_ref.psk8(), rtol=0, atol=1e-15)
    np.testing.assert_allclose(np.array(a16.points), constellation_ref.apsk16(), rtol=0, atol=1e-15)
    # 8PSK: all on the unit circle, Gray around the whole circle, the wrap included
    assert all(abs(abs(p) - 1.0) <= 1e-15 for p in p8.points)
    order = sorted(range(8), key=lambda a: cmath.phase(p8.points[a]) % (2 * math.pi))
    for i in range(8):
        a, b = order[i], order[(i + 1) % 8]
        assert bin(a ^ b).count("1") == 1, (a, b)
        step = (cmath.phase(p8.points[b]) - cmath.phase(p8.points[a])) % (2 * math.pi)
        assert step == pytest.approx(math.pi / 4, abs=1e-14)
    assert cmath.phase(p8.points[0]) == pytest.approx(math.pi / 8, abs=1e-15)  # label 000 -> B = 0
    # 16APSK: 4 + 12 points on two rings in the ratio gamma, label by quadrant
    radii = sorted(abs(p) for p in a16.points)
    assert max(radii[:4]) - min(radii[:4]) <= 1e-15 and max(radii[4:]) - min(radii[4:]) <= 1e-15
    assert radii[4] / radii[0] == pytest.approx(3.15, rel=1e-14)
    assert radii[0] == pytest.approx(math.sqrt(16.0 / (4.0 + 12.0 * 3.15 ** 2)), rel=1e-15)
    for a, p in enumerate(a16.points):
        assert (p.real < 0) == bool(a & 2) and (p.imag < 0) == bool(a & 1), a
    assert cmath.phase(a16.points[0b0100]) == pytest.approx(math.pi / 12, abs=1e-15)
    assert cmath.phase(a16.points[0b1000]) == pytest.approx(5 * math.pi / 12, abs=1e-15)
    assert abs(a16.points[0b1100]) == pytest.approx(radii[0]) and abs(a16.points[0]) == pytest.approx(radii[4])
    for bad in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="gamma"):
            Constellation.apsk16(bad)


def test_from_points_and_from_file(tmp_path):
    raw = [3 + 0j, 0 + 1j, -1 + 0j, 0 - 1j]
    c = Constellation.from_points(raw)
    assert c.name == "custom" and c.bps == 2 and abs(_energy(c) - 1.0) <= 1e-15
    s = 1.0 / math.sqrt((9 + 1 + 1 + 1) / 4.0)
    assert c.points == tuple(p * s for p in raw)
    assert c.flat()[:4] == [3 * s, 0.0, 0.0, s]
    assert c.info() == {"name": "custom", "bps": 2, "points": [[p.real, p.imag] for p in c.points]}
    unit = [cmath.exp(2j * math.pi * i / 4) for i in range(4)]
    assert Constellation.from_points(unit, name="q", normalize=False).points == tuple(unit)
    for pts, normalize, what in ((raw, False, "mean energy"),                        # off energy
                                 ([1, 1j, -1], True, "2\\^bps"),                      # wrong count
                                 ([1], True, "2\\^bps"),
                                 ([1] * 128, True, "2\\^bps"),
                                 ([1, 1j, -1, float("nan")], True, "not finite"),
                                 ([1, 1j, -1, complex(0, float("inf"))], False, "not finite"),
                                 ([1, 1j, 1, -1j], True, "equal"),                     # a duplicate
                                 ([0, 0], True, "zero energy"),
                                 (["a", 1], True, "complex")):
        with pytest.raises(ValueError, match=what):
            Constellation.from_points(pts, normalize=normalize)
    with pytest.raises(ValueError, match="mean energy"):
        Constellation("x", tuple(p * (1 + 1e-8) for p in unit))
    Constellation("x", tuple(p * (1 + 1e-11) for p in unit))  # within the library's 1e-9
    # a file round-trips a table bit for bit
    a16 = Constellation.apsk16()
    path = tmp_path / "apsk.txt"
    a16.to_file(path)
    back = Constellation.from_file(path)
    assert back.points == a16.points and back.name == f"file:{path}"
    path.write_text("# four points\n1 0  # label 0\n\n0 1\n-1 0\n0 -1\n")
    assert Constellation.from_file(path, name="qpsk").points == (1 + 0j, 1j, -1 + 0j, -1j)
    for text, what in (("1 0\n0 1 2\n", "expected `re im`"), ("1 0\nx y\n", "not a pair"), ("1 0\n0 1\n-1 0\n", "2\\^bps"),
                       ("2 0\n0 2\n", "mean energy")):
        path.write_text(text)
        with pytest.raises(ValueError, match=what):
            Constellation.from_file(path)
    with pytest.raises(ValueError, match="constellation file"):
        Constellation.from_file(tmp_path / "missing.txt")
    path.write_text("2 0\n0 2\n")
    assert Constellation.from_file(path, normalize=True).points == (1 + 0j, 1j)


def test_parse_and_effective_bps(tmp_path):
    assert parse("8psk") == Constellation.psk8() and parse("16APSK") == Constellation.apsk16()
    assert parse("16apsk:2.85") == Constellation.apsk16(2.85)
    path = tmp_path / "t.txt"
    Constellation.psk8().to_file(path)
    assert parse(f"file:{path}").points == Constellation.psk8().points
    for bad in ("psk8", "8-psk", "16apsk:x", "16apsk:0.9", "32apsk", f"file:{path}.missing", ""):
        with pytest.raises(ValueError):
            parse(bad)
    qam = ChannelSpec("awgn", "qam16")
    assert effective_bps(qam, None) == 4 and effective_bps(qam, Constellation.psk8()) == 3
    Constellation.psk8().check_length(576)
    with pytest.raises(ValueError, match="n = 7.*bps = 3"):
        Constellation.psk8().check_length(7)


# ------------------------------------------------------------- the library
def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert re.search(r"^#define\s+LDPC_CONST_MAX_BPS\s+6\b", txt, flags=re.M)
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5
    assert "this project's own" in txt  # the built-in labellings claim no standard


_NULL_CALLS = r"""
import ctypes, os
from ldpc_amd import _lib
L = _lib.lib()
pts = (ctypes.c_double * 16)(1, 0, 0, 1, -1, 0, 0, -1)
bps = ctypes.c_int32(-7)
calls = [("set NULL decoder", lambda: L.ldpc_constellation_set(None, 2, pts), b"NULL decoder"),
         ("clear NULL decoder", lambda: L.ldpc_constellation_set(None, 0, None), b"NULL decoder"),
         ("NULL decoder, bad bps", lambda: L.ldpc_constellation_set(None, 7, pts), b"NULL decoder"),
         ("NULL decoder, NULL points", lambda: L.ldpc_constellation_set(None, 3, None), b"NULL decoder"),
         ("get NULL decoder", lambda: L.ldpc_constellation_get(None, ctypes.byref(bps), pts, 16), b"NULL decoder"),
         ("get NULL decoder, NULL bps", lambda: L.ldpc_constellation_get(None, None, None, 0), b"NULL decoder")]
for what, call, msg in calls:
    rc = call()
    assert rc == _lib.LDPC_EINVAL, (what, rc)
    assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
assert bps.value == -7
assert not _lib.hip_started_here()
# no device node was opened: the runtime was never started
opened = [os.readlink(f"/proc/self/fd/{fd}") for fd in os.listdir("/proc/self/fd")
          if os.path.exists(f"/proc/self/fd/{fd}")]
assert not [p for p in opened if p.startswith("/dev/kfd") or p.startswith("/dev/dri")], opened
print("ok")
"""


def test_constellation_set_argument_checks_touch_no_device():
    """In a process of its own: nothing else in it can have started the runtime.
    (The refusals that need a decoder -- a bad bps, NULL points, a coordinate
    that is not finite, the energy, a duplicate, a small capacity -- are in
    tests/test_gpu_constellation.py and, on the host code alone, in
    tools/constellation_host_check.cpp.)"""
    env = dict(os.environ, PYTHONPATH=PKG_DIR + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NULL_CALLS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _links_sanitized(cxx, tmp_path):
    src = tmp_path / "probe.cpp"
    src.write_text("int main() { return 0; }\n")
    exe = str(tmp_path / "probe")
    try:
        ok = subprocess.run([cxx, "-fsanitize=address,undefined", str(src), "-o", exe], capture_output=True,
                            timeout=120).returncode == 0
        return ok and subprocess.run([exe], capture_output=True, timeout=60).returncode == 0
    except (OSError, subprocess.TimeoutExpired):
        return False


def test_library_host_logic_stand_alone(tmp_path):
    """csrc/constellation_host.h (what ldpc_constellation_set validates with and
    what _get copies) in tools/constellation_host_check.cpp, a program of its
    own: built with -Wall -Wextra -Werror, and under the address and
    undefined-behaviour sanitizers where the host compiler links them."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "constellation_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if _links_sanitized(cxx, tmp_path) \
        else []
    print("sanitizers:", "address,undefined" if san else "not linked by this compiler")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", os.path.join(PKG_DIR, "csrc"),
                    os.path.join(ROOT, "tools", "constellation_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "constellation_host_check: OK" in r.stdout, r.stdout + r.stderr


# ---------------------------------------------------- command line and axis
def test_cli_accept_reject_table(capsys, tmp_path):
    head = ["--matrix", "x", "--mode", "physical"]
    a = mc.parse_args(["--matrix", "x"])
    assert a.constellation is None and a.constellation_table is None and a.modulation == "bpsk"
    a = mc.parse_args(head + ["--channel", "awgn", "--constellation", "8psk"])
    assert a.constellation_table == Constellation.psk8() and a.channel_spec == ChannelSpec("awgn") and a.snr_axis == "ebn0"
    a = mc.parse_args(head + ["--channel", "rayleigh", "--constellation", "16apsk:2.57", "--demap", "maxlog",
                              "--fading-block", "7", "--interleaver", "random:7"])
    assert a.constellation_table == Constellation.apsk16(2.57) and a.channel_spec.demap == "maxlog"
    assert mc.parse_args(head + ["--channel", "awgn", "--constellation", "16apsk"]).constellation_table.bps == 4
    path = tmp_path / "t.txt"
    Constellation.from_points([1, 1j, -1, -1j, 2, 2j, -2, -2j]).to_file(path)
    a = mc.parse_args(head + ["--channel", "awgn", "--constellation", f"file:{path}", "--harq", "chase:2"])
    assert a.constellation_table.bps == 3 and a.constellation_table.name == f"file:{path}"
    for argv in (head + ["--constellation", "8psk"],                                        # the reference channel
                 head + ["--channel", "reference", "--constellation", "8psk"],
                 ["--matrix", "x", "--channel", "awgn", "--constellation", "8psk"],          # parity mode
                 ["--matrix", "x", "--mode", "parity", "--channel", "awgn", "--constellation", "8psk"],
                 head + ["--channel", "awgn", "--constellation", "8psk", "--modulation", "qpsk"],
                 head + ["--channel", "awgn", "--constellation", "8psk", "--modulation", "bpsk"],
                 head + ["--channel", "awgn", "--constellation", "psk8"],                    # ChannelSpec's spelling
                 head + ["--channel", "awgn", "--modulation", "psk8"],
                 head + ["--channel", "awgn", "--constellation", "16apsk:1"],
                 head + ["--channel", "awgn", "--constellation", f"file:{path}.missing"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
    assert mc.modulation_header(ChannelSpec("awgn", "qam16"), None) == "modulation qam16"
    assert mc.modulation_header(ChannelSpec("awgn"), Constellation.psk8()) == "constellation 8psk"
    assert "8psk" in mc.constellation_header(Constellation.psk8()) and "bps 3" in mc.constellation_header(Constellation.psk8())


def test_the_ebn0_axis_and_the_checks_use_the_tables_bps():
    awgn, p8, a16 = ChannelSpec("awgn", "qam64"), Constellation.psk8(), Constellation.apsk16()
    want = math.sqrt(1.0 / (2.0 * 0.5 * 3 * 10.0 ** 0.4))
    assert sigma_for_ebn0(4.0, 0.5, 3, table=True) == pytest.approx(want, rel=1e-15)
    assert sigmas_for_axis(awgn, "ebn0", [4.0, 5.0], 0.5, constellation=p8) == \
        [sigma_for_ebn0(4.0, 0.5, 3, table=True), sigma_for_ebn0(5.0, 0.5, 3, table=True)]
    assert sigmas_for_axis(awgn, "ebn0", [4.0], 0.5, constellation=a16) == [sigma_for_ebn0(4.0, 0.5, 4)]
    assert sigmas_for_axis(awgn, "esn0", [4.0], 0.5, constellation=p8) == [sigma_for_esn0(4.0)]
    assert sigmas_for_axis(awgn, "ebn0", [4.0], 0.5) == [sigma_for_ebn0(4.0, 0.5, 6)]  # no table: the modulation's
    for bps in (0, 7):
        with pytest.raises(ValueError):
            sigma_for_ebn0(4.0, 0.5, bps, table=True)
    info = mc.channel_info(awgn, None, [4.0], 0.5, constellation=p8)
    assert info["sigma"] == [sigma_for_ebn0(4.0, 0.5, 3, table=True)] and info["constellation"] == p8.info()
    assert json.loads(json.dumps(info))["constellation"]["bps"] == 3
    assert "constellation" not in mc.channel_info(awgn, None, [4.0], 0.5)
    # E % bps under a pattern: 576 - 6 = 570 = 3 * 190, not a multiple of 4
    from ldpc_amd.ratematch import RateMatch
    rm = RateMatch(tuple(range(570, 576)), ())
    assert mc.rate_match_shape(rm, awgn, 576, 288, p8)[0] == 570
    with pytest.raises(ValueError, match="E = 570.*bps = 4"):
        mc.rate_match_shape(rm, awgn, 576, 288, a16)
    with pytest.raises(ValueError, match="E = 570.*bps = 4"):  # no table: the modulation's
        mc.rate_match_shape(rm, ChannelSpec("awgn", "qam16"), 576, 288)
    assert mc.rate_match_shape(rm, ChannelSpec("awgn", "qam16"), 576, 288, p8)[0] == 570


def test_simulate_refuses_before_any_device_call(monkeypatch):
    """matrix=None: simulate() raises before it loads a code or makes a graph."""
    p8, awgn = Constellation.psk8(), ChannelSpec("awgn")
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, channel=awgn, constellation=p8)
    with pytest.raises(ValueError, match="channel model"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", constellation=p8)
    with pytest.raises(ValueError, match="channel model"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel=ChannelSpec(), constellation=p8)
    with pytest.raises(ValueError, match="Constellation"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel=awgn, constellation="8psk")
    with pytest.raises(ValueError, match="channel model"):
        mc.simulate_harq(None, [0.0], 1, 5, "chase:2", constellation=p8)
    from ldpc_amd import device

    def no_graph(*a, **k):
        raise AssertionError("a graph was made before n was checked against the table's bps")
    monkeypatch.setattr(device, "Graph", no_graph)
    with pytest.raises(ValueError, match="n = 7.*bps = 3"):  # BCH n = 7 under 8PSK
        mc.simulate("BCH_7_4_1_strip", [0.0], 1, 5, mode="physical", channel=awgn, constellation=p8)
    with pytest.raises(ValueError, match="E_r = 100.*bps = 3"):
        mc.simulate_harq("wimax_576_0.5", [0.0], 1, 5, "ir:2:100", channel=awgn, constellation=p8)


# ------------------------------------------------ the restatement's self-checks
@pytest.mark.parametrize("model", ["awgn", "rayleigh"])
@pytest.mark.parametrize("demap", ["exact", "maxlog"])
def test_restatement_on_a_spelled_out_16qam_is_the_channel_restatement(model, demap):
    """Two brute-force formulations (own maxima taken out by hand there, scipy's
    logsumexp here) of the same frame: within the bound the GPU tests use."""
    pts, labels = channel_ref.constellation(4)
    np.testing.assert_array_equal(labels, constellation_ref.label_bits(4))
    c = np.random.default_rng(4).integers(0, 2, 576).astype(np.uint8)
    for sigma in (0.3, 1e-6):
        got, M = constellation_ref.frame_llr(pts, model, demap, c, 20260213, 1000, 3, sigma)
        want, Mw = channel_ref.frame_llr(ChannelSpec(model, "qam16", demap), c, 20260213, 1000, 3, sigma)
        assert M == Mw and np.isfinite(got).all()
        assert (np.abs(got - want) <= 1e-12 * max(1.0, M) + 1e-12 * np.abs(want)).all(), (sigma, np.abs(got - want).max())
    np.testing.assert_array_equal(got > 0, c == 1)  # sigma = 1e-6: the signs are the bits


def test_restatement_composition_and_block_fading():
    """compose() adds the transmissions with their own keys; one transmission in
    column order is frame_llr itself; a coherence length shares the fades."""
    pts = constellation_ref.psk8()
    c = np.random.default_rng(5).integers(0, 2, 24).astype(np.uint8)
    whole, M = constellation_ref.frame_llr(pts, "rayleigh", "exact", c, 7, 3, 1, 0.4)
    llr, bound = constellation_ref.compose(pts, "rayleigh", "exact", c, [np.arange(24)], 7, 3, 1, 0.4)
    np.testing.assert_array_equal(llr, whole)
    np.testing.assert_array_equal(bound, 1e-12 * max(1.0, M) + 1e-12 * np.abs(whole))
    cols = [np.arange(21), np.array([5, 4, 3, 20, 21, 22])]
    first, _ = constellation_ref.frame_llr(pts, "rayleigh", "exact", c[:21], 7, 3, 1, 0.4)
    two, _ = constellation_ref.compose(pts, "rayleigh", "exact", c, cols, 7, 3, 1, 0.4, shortened=(23,))
    again, _ = constellation_ref.frame_llr(pts, "rayleigh", "exact", c[cols[1]], constellation_ref.tx_seed(7, 1), 3, 1, 0.4)
    want = np.zeros(24)
    want[:21] = first
    want[cols[1]] += again
    want[23] = -1.0e4
    np.testing.assert_array_equal(two, want)
    np.testing.assert_array_equal(first, whole[:21])  # the same symbols, the same draws
    assert constellation_ref.tx_seed(2 ** 64 - 1, 1) == 0x9E3779B97F4A7C15 - 1
    # quasi-static: every symbol has the fade of index 0
    h0 = channel_ref.fades(7, 3, 1, 1)[0]
    a, _ = constellation_ref.frame_llr(pts, "rayleigh", "maxlog", c, 7, 3, 1, 0.4, fade_block=8)
    b, _ = constellation_ref.frame_llr(pts * h0, "awgn", "maxlog", c, 7, 3, 1, 0.4)
    np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12)


def test_expected_ber_on_16qam_is_the_closed_form():
    pts, _ = channel_ref.constellation(4)
    for sigma in (0.285, 0.2):
        got = constellation_ref.expected_ber(pts, sigma)
        want = channel_ref.expected_ber(ChannelSpec("awgn", "qam16"), sigma)  # per axis class: a0, a1
        np.testing.assert_allclose(got, np.tile(want, 2), rtol=1e-3, atol=0)


def test_expected_error_rates_of_the_built_in_labellings():
    """Nearest-point decisions, AWGN, per bit position (computed on the CPU with
    the labellings of ldpc_amd/constellation.py)."""
    got = constellation_ref.expected_ber(constellation_ref.psk8(), 0.30)
    print("8psk, sigma 0.30:", got)
    np.testing.assert_allclose(got, [0.051, 0.051, 0.100], rtol=0, atol=0.003)
    got = constellation_ref.expected_ber(constellation_ref.apsk16(3.15), 0.25)
    print("16apsk(3.15), sigma 0.25:", got)
    np.testing.assert_allclose(got, [0.095, 0.095, 0.069, 0.069], rtol=0, atol=0.003)
