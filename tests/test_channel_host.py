"""Host side of the physical-mode channel models (ldpc_channel_set /
ldpc_channel_get, ldpc_amd.channel): the SNR axes, the spec's validation, the
command line, simulate()'s refusals, the argument checks that need no device,
the header, and the self-checks of the numpy restatement (tests/channel_ref.py).
No GPU."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import channel_ref
from conftest import PKG_DIR, ROOT
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import (ChannelSpec, reference_axis_as_ebn0, resolve_snr_axis, sigma_for_ebn0, sigma_for_esn0,
                              sigmas_for_axis)

NEW = ("ldpc_channel_set", "ldpc_channel_get")
SEED = 20260213


def test_sigma_hand_values():
    assert sigma_for_esn0(0.0) == pytest.approx(math.sqrt(0.5), rel=1e-15)
    assert sigma_for_esn0(10.0) == pytest.approx(math.sqrt(0.05), rel=1e-15)
    # rate 1/2 BPSK at Eb/N0 = 0 dB: Es/N0 = 1/2, sigma^2 = 1
    assert sigma_for_ebn0(0.0, 0.5, 1) == pytest.approx(1.0, rel=1e-15)
    # rate 1/2 QPSK: Es = Eb, the same as Es/N0
    assert sigma_for_ebn0(3.0, 0.5, 2) == pytest.approx(sigma_for_esn0(3.0), rel=1e-15)
    # rate 3/4 64-QAM at 10 dB: 1 / (2 * 0.75 * 6 * 10) = 1/90
    assert sigma_for_ebn0(10.0, 0.75, 6) == pytest.approx(math.sqrt(1.0 / 90.0), rel=1e-15)
    assert sigma_for_ebn0(2.0, 0.5, 4) == pytest.approx(math.sqrt(1.0 / (2 * 0.5 * 4 * 10 ** 0.2)), rel=1e-15)
    for bad in ((0.0, 0.0, 1), (0.0, 1.5, 1), (0.0, 0.5, 3)):
        with pytest.raises(ValueError):
            sigma_for_ebn0(*bad)


def test_reference_axis_worked_example():
    """The "-2.5 dB" waterfall of wimax_2304_0.5 on the reference axis: noise
    standard deviation sigma^2 = 0.889, Es/N0 = -1.99 dB, Eb/N0 = +1.0 dB."""
    sigma = mc.sigma_for_snr(-2.5)
    std, esn0, ebn0 = reference_axis_as_ebn0(-2.5, 0.5)
    assert std == pytest.approx(sigma * sigma, rel=1e-15)
    assert round(std, 3) == 0.889 and round(esn0, 2) == -1.99 and round(ebn0, 2) == 1.02
    # a textbook BPSK channel at that Eb/N0 has exactly that noise
    assert sigma_for_ebn0(ebn0, 0.5, 1) == pytest.approx(std, rel=1e-12)


def test_channel_spec_validation():
    assert ChannelSpec() == ChannelSpec("reference", "bpsk", "exact") and ChannelSpec().is_reference
    assert ChannelSpec("rayleigh", "qam16", "maxlog").codes() == (2, 4, 1)
    assert ChannelSpec("awgn", "qam64").codes() == (1, 6, 0) and ChannelSpec("awgn", "qpsk").bps == 2
    assert ChannelSpec.from_codes(1, 6, 1) == ChannelSpec("awgn", "qam64", "maxlog")
    for bad in (("awgm",), ("awgn", "psk8"), ("awgn", "qpsk", "approx"), ("reference", "qpsk"),
                ("reference", "qam64", "maxlog")):
        with pytest.raises(ValueError):
            ChannelSpec(*bad)
    ChannelSpec("awgn", "qam64").check_length(576)
    with pytest.raises(ValueError, match="66.*bps = 4"):
        ChannelSpec("awgn", "qam16").check_length(66)
    ChannelSpec().check_length(7)  # the reference channel takes any n


def test_snr_axis_rules():
    ref, awgn = ChannelSpec(), ChannelSpec("awgn", "qam16")
    assert resolve_snr_axis(None) == "reference" and resolve_snr_axis(ref, "reference") == "reference"
    assert resolve_snr_axis(awgn) == "ebn0" and resolve_snr_axis(awgn, "esn0") == "esn0"
    for spec, axis in ((ref, "esn0"), (ref, "ebn0"), (awgn, "reference"), (awgn, "snr")):
        with pytest.raises(ValueError):
            resolve_snr_axis(spec, axis)
    assert sigmas_for_axis(ref, "reference", [0.0, -2.5], 0.5) == [mc.sigma_for_snr(0.0), mc.sigma_for_snr(-2.5)]
    assert sigmas_for_axis(awgn, "ebn0", [4.0], 0.5) == [sigma_for_ebn0(4.0, 0.5, 4)]
    assert sigmas_for_axis(awgn, "esn0", [4.0], 0.5) == [sigma_for_esn0(4.0)]


def test_cli_accept_reject_table(capsys):
    head = ["--matrix", "x"]
    a = mc.parse_args(head)  # the defaults: today's run
    assert (a.channel, a.modulation, a.demap, a.snr_axis) == ("reference", "bpsk", "exact", "reference")
    assert a.channel_spec.is_reference
    phys = ["--mode", "physical", "--cn-rule", "nms", "--schedule", "layered"]
    a = mc.parse_args(head + phys + ["--channel", "awgn", "--modulation", "qam16"])
    assert a.channel_spec == ChannelSpec("awgn", "qam16", "exact") and a.snr_axis == "ebn0"
    a = mc.parse_args(head + phys + ["--channel", "rayleigh", "--modulation", "qam64", "--demap", "maxlog",
                                     "--snr-axis", "esn0"])
    assert a.channel_spec == ChannelSpec("rayleigh", "qam64", "maxlog") and a.snr_axis == "esn0"
    a = mc.parse_args(head + ["--mode", "physical", "--channel", "awgn"])
    assert a.channel_spec == ChannelSpec("awgn") and a.snr_axis == "ebn0"
    assert mc.parse_args(head + phys + ["--snr-axis", "reference"]).snr_axis == "reference"
    for argv in (["--channel", "awgn"],                                              # no --mode physical
                 ["--mode", "parity", "--channel", "rayleigh", "--modulation", "qpsk"],
                 phys + ["--modulation", "qpsk"],                                    # the reference channel is BPSK
                 phys + ["--channel", "reference", "--modulation", "qam16"],
                 phys + ["--demap", "maxlog"],                                       # nothing to demap
                 phys + ["--snr-axis", "ebn0"],                                      # the reference has its own axis
                 ["--snr-axis", "esn0"],
                 phys + ["--channel", "awgn", "--snr-axis", "reference"],
                 phys + ["--channel", "awgn", "--modulation", "psk8"],
                 phys + ["--channel", "fading"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_simulate_refuses_before_any_device_call():
    """matrix=None: simulate() raises before it loads a code or makes a graph."""
    qam = ChannelSpec("awgn", "qam16")
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, channel=qam)
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, mode="parity", channel=ChannelSpec("rayleigh"), snr_axis="ebn0")
    with pytest.raises(ValueError, match="reference"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", cn_rule="nms", channel=qam, snr_axis="reference")
    with pytest.raises(ValueError, match="reference"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", snr_axis="ebn0")
    with pytest.raises(ValueError, match="snr_axis"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel=qam, snr_axis="cn0")
    with pytest.raises(ValueError, match="ChannelSpec"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", channel="awgn")


def test_simulate_refuses_a_length_that_does_not_divide(monkeypatch):
    """BCH n = 7 under QPSK: refused when the code is known, before a graph is made."""
    from ldpc_amd import device

    def no_graph(*a, **k):
        raise AssertionError("simulate() made a graph before it checked n against bps")
    monkeypatch.setattr(device, "Graph", no_graph)
    with pytest.raises(ValueError, match="n = 7.*bps = 2"):
        mc.simulate("BCH_7_4_1_strip", [0.0], 1, 5, mode="physical", channel=ChannelSpec("awgn", "qpsk"))


def test_channel_info_document():
    info = mc.channel_info(ChannelSpec("awgn", "qam16", "maxlog"), None, [1.0, 2.0], 0.5)
    assert info == {"model": "awgn", "modulation": "qam16", "demap": "maxlog", "snr_axis": "ebn0",
                    "sigma": [sigma_for_ebn0(1.0, 0.5, 4), sigma_for_ebn0(2.0, 0.5, 4)]}
    assert mc.channel_info(None, None, [0.0], 0.5)["sigma"] == [mc.sigma_for_snr(0.0)]


def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    for define in ("LDPC_CH_REFERENCE 0", "LDPC_CH_AWGN 1", "LDPC_CH_RAYLEIGH 2", "LDPC_DEMAP_EXACT 0",
                   "LDPC_DEMAP_MAXLOG 1"):
        assert re.search(rf"^#define\s+{define}\b", txt, flags=re.M), define
    assert re.search(r"int32_t model, modulation, demap, reserved;\s*\}\s*ldpc_channel;", txt)
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5


_NULL_CALLS = r"""
import ctypes, os
from ldpc_amd import _lib
L = _lib.lib()
def ch(*v):
    return ctypes.byref(_lib.Channel(*v))
calls = [("NULL decoder", lambda: L.ldpc_channel_set(None, ch(1, 4, 0, 0)), b"NULL decoder"),
         ("NULL decoder, NULL channel", lambda: L.ldpc_channel_set(None, None), b"NULL decoder"),
         ("get NULL", lambda: L.ldpc_channel_get(None, ch(0, 1, 0, 0)), b"NULL decoder"),
         ("bad model", lambda: L.ldpc_channel_set(None, ch(3, 1, 0, 0)), b"model 3"),
         ("negative model", lambda: L.ldpc_channel_set(None, ch(-1, 1, 0, 0)), b"model -1"),
         ("bad modulation", lambda: L.ldpc_channel_set(None, ch(1, 3, 0, 0)), b"modulation 3"),
         ("8 bits per symbol", lambda: L.ldpc_channel_set(None, ch(2, 8, 0, 0)), b"modulation 8"),
         ("bad demap", lambda: L.ldpc_channel_set(None, ch(1, 4, 2, 0)), b"demap 2"),
         ("reserved", lambda: L.ldpc_channel_set(None, ch(1, 4, 0, 7)), b"reserved"),
         ("REFERENCE + QPSK", lambda: L.ldpc_channel_set(None, ch(0, 2, 0, 0)), b"BPSK")]
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


def test_channel_set_argument_checks_touch_no_device():
    """In a process of its own: nothing else in it can have started the runtime."""
    env = dict(os.environ, PYTHONPATH=PKG_DIR + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NULL_CALLS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


# ------------------------------------------------ the restatement's self-checks
def _level(bits, bps):
    """The contract's formula: b0 = a0, b_i = b_(i-1) xor a_i, B = sum b_i 2^(m-1-i), (2B - (2^m - 1)) d."""
    m = len(bits)
    b, B = 0, 0
    for a in bits:
        b ^= int(a)
        B = 2 * B + b
    return (2 * B - (2 ** m - 1)) * channel_ref.SCALE[bps]


def test_gray_tables_equal_the_formula():
    for bps, m in ((2, 1), (4, 2), (6, 3)):
        pts, labels = channel_ref.constellation(bps)
        assert len(pts) == 2 ** bps == len({complex(p) for p in pts})
        for p, lab in zip(pts, labels):
            assert p.real == pytest.approx(_level(lab[:m], bps), abs=1e-15)
            assert p.imag == pytest.approx(_level(lab[m:], bps), abs=1e-15)
        # Gray: neighbours on an axis differ in one bit
        table = channel_ref.AXIS_LEVELS[m]
        order = sorted(table, key=table.get)
        assert [table[a] for a in order] == list(range(-(2 ** m - 1), 2 ** m, 2))
        assert all(sum(x != y for x, y in zip(a, b)) == 1 for a, b in zip(order, order[1:]))
    pts, labels = channel_ref.constellation(1)
    assert list(pts) == [-1.0, 1.0] and labels.tolist() == [[0], [1]]
    # the examples the contract writes out
    assert channel_ref.AXIS_LEVELS[2][(1, 1)] == 1 and channel_ref.AXIS_LEVELS[2][(1, 0)] == 3
    assert channel_ref.AXIS_LEVELS[3][(0, 1, 0)] == -1 and channel_ref.AXIS_LEVELS[3][(1, 0, 0)] == 7


@pytest.mark.parametrize("bps", [1, 2, 4, 6])
def test_unit_average_energy(bps):
    pts, _ = channel_ref.constellation(bps)
    assert np.mean(np.abs(pts) ** 2) == pytest.approx(1.0, rel=1e-14)
    assert abs(pts.mean()) < 1e-15


def _bits(n, seed):
    return np.random.default_rng(seed).integers(0, 2, n).astype(np.uint8)


def test_bpsk_awgn_is_two_y_over_sigma_squared():
    n, sigma, F = 96, 0.8, 1234
    c = _bits(n, 1)
    llr, M = channel_ref.frame_llr(ChannelSpec("awgn"), c, SEED, F, 3, sigma)
    g = channel_ref.noise_pairs(SEED, F, 3, n // 2).reshape(-1)
    y = (2.0 * c - 1.0) + sigma * g
    np.testing.assert_allclose(llr, 2.0 * y / sigma ** 2, rtol=0, atol=1e-12 * max(1.0, M))
    ml, _ = channel_ref.frame_llr(ChannelSpec("awgn", demap="maxlog"), c, SEED, F, 3, sigma)
    np.testing.assert_allclose(ml, llr, rtol=0, atol=1e-12 * max(1.0, M))


def test_noise_draws_are_the_frame_sources():
    """The restatement's noise is the committed frame source's: under the
    reference channel llr = 2 (x + s^2 g) / s^2 reproduces oracle.generate_frames."""
    import oracle
    from conftest import hstd_for
    H = hstd_for("wimax_576_0.5")
    sigma = 0.9
    _, c, llr = oracle.generate_frames(H, SEED, 3, sigma, 1000, 2)
    for f in range(2):
        g = channel_ref.noise_pairs(SEED, 1000 + f, 3, 288).reshape(-1)
        s2 = sigma * sigma
        np.testing.assert_allclose(2.0 * ((2.0 * c[f] - 1.0) + s2 * g) / s2, llr[f], rtol=1e-13, atol=0)


@pytest.mark.parametrize("model", ["awgn", "rayleigh"])
@pytest.mark.parametrize("mod", ["qpsk", "qam16", "qam64"])
def test_exact_tends_to_maxlog_as_sigma_vanishes(model, mod):
    """exact - max-log = log of sums of exp(-(mu - min)) <= log(2^(bps-1)); as
    sigma -> 0 the metrics separate and the difference, relative to the LLR, vanishes."""
    bps = ChannelSpec(model, mod).bps
    c = _bits(24 * bps, 2)
    rel = []
    for sigma in (0.3, 0.03, 0.003):
        ex, _ = channel_ref.frame_llr(ChannelSpec(model, mod, "exact"), c, SEED, 77, 0, sigma)
        ml, _ = channel_ref.frame_llr(ChannelSpec(model, mod, "maxlog"), c, SEED, 77, 0, sigma)
        assert np.all(np.abs(ex - ml) <= math.log(2 ** (bps - 1)) + 1e-9)
        assert np.array_equal(np.sign(ex), np.sign(ml)) or sigma == 0.3
        rel.append(float(np.max(np.abs(ex - ml) / np.abs(ml))))
    # (QPSK: the other axis cancels, the two agree at every sigma; far apart the exponentials underflow to 0)
    assert rel[0] >= rel[1] >= rel[2] and rel[2] < 1e-3 and (bps == 2 or rel[0] > 1e-3)


def test_signs_follow_the_bits_without_noise():
    """At a vanishing sigma every LLR carries its bit's sign (positive = bit 1)."""
    for spec in (ChannelSpec("awgn", "bpsk"), ChannelSpec("rayleigh", "qpsk"), ChannelSpec("awgn", "qam16"),
                 ChannelSpec("rayleigh", "qam64", "maxlog")):
        c = _bits(48 * spec.bps, 3)
        llr, _ = channel_ref.frame_llr(spec, c, SEED, 5, 1, 1e-3)
        assert np.array_equal(llr > 0, c == 1), spec


def test_expected_ber_closed_forms():
    q = channel_ref._q
    s = 0.7
    assert channel_ref.expected_ber(ChannelSpec("awgn", "bpsk"), s)[0] == pytest.approx(q(1 / s), rel=1e-12)
    assert channel_ref.expected_ber(ChannelSpec("awgn", "qpsk"), s)[0] == pytest.approx(q(math.sqrt(0.5) / s), rel=1e-12)
    # 16-QAM: a0 = (Q(d/s) + Q(3d/s)) / 2,  a1 = Q(d/s) + (Q(3d/s) - Q(5d/s)) / 2
    d = 1 / math.sqrt(10)
    e = channel_ref.expected_ber(ChannelSpec("awgn", "qam16"), 0.3)
    assert e[0] == pytest.approx(0.5 * (q(d / 0.3) + q(3 * d / 0.3)), rel=1e-12)
    assert e[1] == pytest.approx(q(d / 0.3) + 0.5 * (q(3 * d / 0.3) - q(5 * d / 0.3)), rel=1e-12)
    # Rayleigh BPSK with E[h^2] = 1: (1 - sqrt(g / (1 + g))) / 2, g = 1 / (2 s^2)
    g = 1 / (2 * s * s)
    assert channel_ref.expected_ber(ChannelSpec("rayleigh", "bpsk"), s)[0] == \
        pytest.approx(0.5 * (1 - math.sqrt(g / (1 + g))), rel=1e-8)
    assert channel_ref.bit_classes(6, 12).tolist() == [0, 1, 2, 0, 1, 2] * 2
    assert channel_ref.bit_classes(1, 3).tolist() == [0, 0, 0] and channel_ref.bit_classes(2, 4).tolist() == [0] * 4
