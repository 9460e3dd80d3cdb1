"""Host side of the physical-mode bit interleaver and block fading
(ldpc_interleaver_set / _get, ldpc_fading_set / _get, ldpc_amd.interleave): the
builders' pinned values, the command line's grammar, simulate()'s refusals, the
argument checks that need no device, the header, the stats-json object, the
library's host logic as a stand-alone program, and the numpy restatement's own
identities (tests/interleave_ref.py).  No GPU."""
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG_DIR, ROOT, hstd_for
from ldpc_amd import _lib
from ldpc_amd import interleave as il
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec
from ldpc_amd.ratematch import RateMatch

NEW = ("ldpc_interleaver_set", "ldpc_interleaver_get", "ldpc_fading_set", "ldpc_fading_get")
RM_W576 = RateMatch(tuple(288 + 6 * i for i in range(48)), tuple(range(24)))  # E = 504
SEED = 20260213


def _is_perm(p):
    return sorted(p) == list(range(len(p)))


# ------------------------------------------------------------ the builders
def test_splitmix64_and_random_pinned_values():
    assert il.SplitMix64(0).next() == 0xE220A8397B1DCDAF
    assert list(il.random(8, 1).perm) == [4, 3, 2, 7, 5, 6, 0, 1]
    assert list(il.random(12, 20260213).perm) == [2, 4, 9, 11, 6, 8, 5, 0, 3, 1, 7, 10]
    assert list(il.random(57, 7).perm[:10]) == [7, 4, 20, 36, 54, 25, 34, 8, 16, 0]
    assert il.random(8).perm == il.random(8, 0).perm and il.random(8, 1).perm != il.random(8, 2).perm
    assert il.random(1, 5).perm == (0,)


def test_regular_shapes_and_block_hand_values():
    for E, shape in ((576, (24, 24)), (504, (21, 24)), (2304, (48, 48)), (1248, (32, 39)), (57, (3, 19)),
                     (52, (4, 13)), (53, (1, 53))):
        assert il.regular_shape(E) == shape, E
        r = il.regular(E)
        assert r.perm == il.block(E, shape[0]).perm and r.kind == "regular"
        assert r.info() == {"kind": "regular", "length": E, "rows": shape[0], "cols": shape[1]}
    assert il.regular(53).is_identity and il.regular(53).perm == il.identity(53).perm
    assert list(il.block(6, 2).perm) == [0, 3, 1, 4, 2, 5]
    assert list(il.block(6, 3).perm) == [0, 2, 4, 1, 3, 5]
    assert il.block(6, 1).is_identity and il.block(6, 6).is_identity
    # pi[c * rows + r] = r * C + c
    b = il.block(504, 21)
    assert all(b.perm[c * 21 + r] == r * 24 + c for r in range(21) for c in range(24))
    for E, rows in ((6, 4), (6, 0), (6, -2), (6, 7), (6, 1.5)):
        with pytest.raises(ValueError):
            il.block(E, rows)


def test_every_builder_returns_a_permutation(tmp_path):
    path = tmp_path / "perm.txt"
    path.write_text("3 1\n4 0\t2\n")
    built = [il.identity(57), il.block(504, 21), il.regular(576), il.regular(57), il.random(504, 7),
             il.random(57, 7), il.srandom(1248, 12, 3), il.srandom(57, 5, 0), il.srandom(576, 0, 1),
             il.from_file(str(path)), il.parse("random:3", 64), il.parse(f"file:{path}", 5)]
    for b in built:
        assert _is_perm(b.perm) and len(b) == len(b.perm), b.kind
        assert b.validate(len(b)) is b
        with pytest.raises(ValueError, match="length"):
            b.validate(len(b) + 1)
    assert il.from_file(str(path)).perm == (3, 1, 4, 0, 2)
    assert il.identity(4).perm == (0, 1, 2, 3) and il.identity(4).is_identity and not il.random(8, 1).is_identity
    # the class validates what the library validates
    for bad in ((0, 1, 3), (0, -1, 2), (1, 1, 0), "012", (0.5, 1), ("a",)):
        with pytest.raises(ValueError):
            il.Interleaver(bad)
    with pytest.raises(Exception):
        built[0].perm = ()  # frozen
    for E in (0, -3, 2.5):
        with pytest.raises(ValueError):
            il.identity(E)
    for text in ("", "1 2 x", "0 0 1"):
        path.write_text(text)
        with pytest.raises(ValueError):
            il.from_file(str(path))


def test_srandom_distance_property_and_determinism():
    for E, S, seed in ((1248, 12, 3), (504, 8, 0), (57, 5, 1), (576, 10, 20260213)):
        p = il.srandom(E, S, seed).perm
        assert _is_perm(p)
        worst = min(abs(p[i] - p[j]) for i in range(E) for j in range(max(0, i - S), i))
        assert worst > S, (E, S, seed, worst)
        assert il.s_distance_ok(p, S)
        assert il.srandom(E, S, seed).perm == p                  # a function of (E, S, seed)
    assert il.srandom(504, 8, 0).perm != il.srandom(504, 8, 1).perm
    assert il.srandom(504, 8).perm == il.srandom(504, 8, 0).perm
    assert not il.s_distance_ok(il.identity(16).perm, 1) and il.s_distance_ok(il.identity(16).perm, 0)
    assert il.srandom(1248, 12, 3).info() == {"kind": "srandom", "length": 1248, "S": 12, "seed": 3}
    for E, S in ((57, 6), (1248, 25), (8, 3), (57, -1), (57, 1.5)):  # floor(sqrt(57 / 2)) = 5, of 624: 24
        with pytest.raises(ValueError):
            il.srandom(E, S)


# ------------------------------------------------------------ the grammar
def test_parse_accept_reject_table(tmp_path):
    assert il.parse("none", 576) is None and il.parse(" None ", 576) is None
    assert il.parse("regular", 576).perm == il.regular(576).perm
    assert il.parse("block:24", 576).perm == il.block(576, 24).perm
    assert il.parse("block: 2", 6).perm == (0, 3, 1, 4, 2, 5)
    assert il.parse("random", 57).perm == il.random(57, 0).perm
    assert il.parse("random:7", 57).perm == il.random(57, 7).perm
    assert il.parse("srandom:5", 57).perm == il.srandom(57, 5, 0).perm
    assert il.parse("srandom:5:1", 57).perm == il.srandom(57, 5, 1).perm
    path = tmp_path / "p.txt"
    path.write_text("2 0 1")
    assert il.parse(f"file:{path}", 3).perm == (2, 0, 1)
    with pytest.raises(ValueError, match="length"):
        il.parse(f"file:{path}", 4)
    with pytest.raises((ValueError, OSError)):
        il.parse(f"file:{path}.missing", 3)
    for bad in ("", " ", "foo", "regular:3", "none:1", "block", "block:", "block:x", "block:2:3", "block:5", "block:0",
                "random:", "random:x", "random:1:2", "srandom", "srandom:x", "srandom:1:2:3", "srandom:99", "file:",
                "24", ":", "block::2"):
        with pytest.raises(ValueError):
            il.parse(bad, 576)
    with pytest.raises(ValueError):
        il.parse(7, 576)
    assert il.resolve(None, 576) is None and il.resolve("none", 576) is None
    assert il.resolve("regular", 504).perm == il.regular(504).perm
    r = il.random(504, 7)
    assert il.resolve(r, 504) is r
    with pytest.raises(ValueError, match="length"):
        il.resolve(r, 576)
    with pytest.raises(ValueError):
        il.resolve((0, 1, 2), 3)


def test_cli_accept_reject_table(capsys):
    head = ["--matrix", "wimax_576_0.5"]
    phys = ["--mode", "physical", "--cn-rule", "nms", "--schedule", "layered"]
    ray = phys + ["--channel", "rayleigh", "--modulation", "qam16"]
    a = mc.parse_args(head)
    assert a.interleaver is None and a.fading_block == 1
    a = mc.parse_args(head + ray)
    assert a.interleaver is None and a.fading_block == 1
    a = mc.parse_args(head + ray + ["--fading-block", "24", "--interleaver", "regular"])
    assert a.interleaver == "regular" and a.fading_block == 24
    a = mc.parse_args(head + ray + ["--fading-block", "frame", "--interleaver", "random:7"])
    assert a.interleaver == "random:7" and a.fading_block == mc.FADING_FRAME
    a = mc.parse_args(head + ray + ["--interleaver", "none", "--fading-block", "1"])
    assert a.interleaver is None and a.fading_block == 1
    a = mc.parse_args(head + phys + ["--channel", "awgn", "--modulation", "qam64", "--interleaver", "srandom:12:3"])
    assert a.interleaver == "srandom:12:3"
    for argv in (["--interleaver", "regular"],                                     # no --mode physical
                 phys + ["--interleaver", "regular"],                             # the reference channel
                 phys + ["--channel", "reference", "--interleaver", "random"],
                 ["--mode", "parity", "--fading-block", "4"],
                 phys + ["--fading-block", "4"],
                 phys + ["--channel", "awgn", "--fading-block", "4"],             # no fade to share
                 ray + ["--fading-block", "0"], ray + ["--fading-block", "-3"], ray + ["--fading-block", "x"],
                 ray + ["--fading-block", "2.5"], ray + ["--fading-block", str(2 ** 31)],
                 ray + ["--interleaver", "foo"], ray + ["--interleaver", "block"], ray + ["--interleaver", "block:x"],
                 ray + ["--interleaver", "random:1:2"], ray + ["--interleaver", "file:"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_cli_refuses_before_any_device_call(monkeypatch, capsys):
    """main() turns an interleaver the code cannot carry into an exit before simulate() is reached."""
    def no_simulate(*a, **k):
        raise AssertionError("main() reached simulate() with an interleaver it should have refused")
    monkeypatch.setattr(mc, "simulate", no_simulate)
    base = ["--matrix", "wimax_576_0.5", "--mode", "physical", "--channel", "rayleigh", "--modulation", "qam16"]
    with pytest.raises(SystemExit, match="divisor"):
        mc.main(base + ["--interleaver", "block:5"])
    with pytest.raises(SystemExit, match="sqrt"):
        mc.main(base + ["--interleaver", "srandom:17"])
    with pytest.raises(SystemExit, match="interleaver"):
        mc.main(base + ["--interleaver", "file:/nonexistent/permutation"])


def test_simulate_refuses_before_any_device_call(monkeypatch, tmp_path):
    """matrix=None: simulate() raises before it loads a code or makes a graph."""
    qam = ChannelSpec("awgn", "qam16")
    ray = ChannelSpec("rayleigh", "qam16")
    for kw, msg in ((dict(interleaver="regular"), "physical"),
                    (dict(mode="physical", interleaver="regular"), "channel model"),
                    (dict(mode="physical", channel=ChannelSpec(), interleaver=il.regular(576)), "channel model"),
                    (dict(mode="physical", channel=qam, interleaver=(0, 1, 2)), "Interleaver"),
                    (dict(mode="physical", channel=qam, interleaver="foo"), "spec"),
                    (dict(mode="physical", channel=qam, interleaver="block"), "spec"),
                    (dict(fading_block=4), "physical"),
                    (dict(mode="physical", fading_block=4), "Rayleigh"),
                    (dict(mode="physical", channel=qam, fading_block=4), "Rayleigh"),
                    (dict(mode="physical", channel=ray, fading_block=0), "fading_block"),
                    (dict(mode="physical", channel=ray, fading_block=-1), "fading_block"),
                    (dict(mode="physical", channel=ray, fading_block=2.0), "fading_block"),
                    (dict(mode="physical", channel=ray, fading_block=True), "fading_block"),
                    (dict(mode="physical", channel=ray, fading_block="block"), "fading_block"),
                    (dict(mode="physical", channel=ray, fading_block=2 ** 31), "fading_block")):
        with pytest.raises(ValueError, match=msg):
            mc.simulate(None, [0.0], 1, 5, **kw)
    # once the code and the pattern are known: before a graph is made
    from ldpc_amd import device

    def no_graph(*a, **k):
        raise AssertionError("simulate() made a graph before it checked the interleaver")
    monkeypatch.setattr(device, "Graph", no_graph)
    W = "wimax_576_0.5"
    for kw, msg in ((dict(interleaver=il.regular(504)), "length 504.*E = 576"),
                    (dict(interleaver=il.regular(576), rate_match=RM_W576), "length 576.*E = 504"),
                    (dict(interleaver="block:5"), "divisor"),
                    (dict(interleaver="block:16", rate_match=RM_W576), "divisor of E = 504"),  # 16 divides 576, not 504
                    (dict(interleaver="srandom:17"), "sqrt"),
                    (dict(interleaver=f"file:{tmp_path}/missing"), None)):
        with pytest.raises((ValueError, OSError), match=msg):
            mc.simulate(W, [0.0], 1, 5, mode="physical", channel=ray, **kw)
    with pytest.raises(ValueError, match="length 576.*E = 1440"):
        mc.simulate("ira_1440_0.5", [0.0], 1, 5, mode="physical", cn_rule="nms", channel=qam,
                    interleaver=il.regular(576))
    # what is acceptable gets as far as the graph
    for kw in (dict(interleaver="regular", fading_block=24), dict(interleaver="random:7", fading_block="frame"),
               dict(interleaver="block:21", rate_match=RM_W576), dict(interleaver="none"), dict(fading_block=1)):
        with pytest.raises(AssertionError, match="made a graph"):
            mc.simulate(W, [0.0], 1, 5, mode="physical", channel=ray, **kw)
    assert mc.check_interleave_args(None, 1, None, "parity") == (None, 1)
    assert mc.check_interleave_args("none", 1, None, "parity") == (None, 1)
    assert mc.check_interleave_args("regular", "frame", ray, "physical") == ("regular", mc.FADING_FRAME)


def test_stats_json_objects_and_header(tmp_path):
    spec = ChannelSpec("rayleigh", "qam16")
    plain = mc.channel_info(spec, None, [6.0], 0.5)
    assert "interleaver" not in plain and "fading_block" not in plain
    assert mc.channel_info(spec, None, [6.0], 0.5, None, None, None, None, 1) == plain  # unchanged when nothing is set
    info = mc.channel_info(spec, None, [6.0], 0.5, None, 576, 288, il.regular(576), 24)
    assert info["interleaver"] == {"kind": "regular", "length": 576, "rows": 24, "cols": 24}
    assert info["fading_block"] == 24
    assert {k: v for k, v in info.items() if k not in ("interleaver", "fading_block")} == plain
    only_il = mc.channel_info(spec, None, [6.0], 0.5, interleaver=il.random(576, 7))
    assert only_il["interleaver"] == {"kind": "random", "length": 576, "seed": 7} and "fading_block" not in only_il
    frame = mc.channel_info(spec, None, [6.0], 0.5, fading_block=mc.FADING_FRAME)
    assert frame["fading_block"] == "frame" and "interleaver" not in frame
    st = mc.reduce_stats([{"hist": np.array([0, 3, 1]), "undetected_frames": 0, "undetected_bit_errors": 0,
                           "failed": np.zeros((0, 2), np.int64), "failed_dropped": 1}], [6.0])
    path = tmp_path / "s.json"
    mc.stats_to_json(str(path), 7, st, channel=info)
    doc = json.loads(path.read_text())
    assert doc["channel"]["interleaver"]["rows"] == 24 and doc["channel"]["fading_block"] == 24
    head = mc.interleave_header(info)
    assert "interleaver" in head and "regular" in head and "rows 24" in head and "coherence length 24" in head
    assert "coherence length frame" in mc.interleave_header(frame) and "interleaver none" in mc.interleave_header(frame)
    assert "random" in mc.interleave_header(only_il) and "coherence length 1 " in mc.interleave_header(only_il)


# ------------------------------------------------------------ the library
def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert "0, 3, 1, 4, 2, 5" in txt  # the worked example
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5


_NULL_CALLS = r"""
import ctypes, os
from ldpc_amd import _lib
L = _lib.lib()
perm = (ctypes.c_int32 * 3)(2, 0, 1)
n = ctypes.c_int32(77)
calls = [("set NULL decoder", lambda: L.ldpc_interleaver_set(None, 3, perm), b"NULL decoder"),
         ("set NULL decoder, clearing", lambda: L.ldpc_interleaver_set(None, 0, None), b"NULL decoder"),
         ("set NULL decoder, bad length", lambda: L.ldpc_interleaver_set(None, -1, None), b"NULL decoder"),
         ("set NULL decoder, NULL perm", lambda: L.ldpc_interleaver_set(None, 3, None), b"NULL decoder"),
         ("get NULL decoder", lambda: L.ldpc_interleaver_get(None, ctypes.byref(n), None, 0), b"NULL decoder"),
         ("get NULL decoder, NULL len", lambda: L.ldpc_interleaver_get(None, None, perm, 3), b"NULL decoder"),
         ("fading NULL decoder", lambda: L.ldpc_fading_set(None, 4), b"NULL decoder"),
         ("fading NULL decoder, bad length", lambda: L.ldpc_fading_set(None, 0), b"NULL decoder"),
         ("fading get NULL decoder", lambda: L.ldpc_fading_get(None, ctypes.byref(n)), b"NULL decoder"),
         ("fading get NULL both", lambda: L.ldpc_fading_get(None, None), b"NULL decoder")]
for what, call, msg in calls:
    rc = call()
    assert rc == _lib.LDPC_EINVAL, (what, rc)
    assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
assert n.value == 77 and list(perm) == [2, 0, 1]
assert not _lib.hip_started_here()
# no device node was opened: the runtime was never started
opened = [os.readlink(f"/proc/self/fd/{fd}") for fd in os.listdir("/proc/self/fd")
          if os.path.exists(f"/proc/self/fd/{fd}")]
assert not [p for p in opened if p.startswith("/dev/kfd") or p.startswith("/dev/dri")], opened
print("ok")
"""


def test_argument_checks_touch_no_device():
    """In a process of its own: nothing else in it can have started the runtime."""
    env = dict(os.environ, PYTHONPATH=PKG_DIR + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NULL_CALLS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def _links_sanitized(cxx, tmp_path):
    """Whether the host compiler links an address + undefined-behaviour sanitized program that runs."""
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
    """csrc/rate_match_host.h (what ldpc_interleaver_set validates with, the
    composite table the kernels gather and scatter with, and the gate before its
    upload) in tools/interleave_host_check.cpp, a program of its own: built
    with -Wall -Wextra -Werror, and under the address and undefined-behaviour
    sanitizers where the host compiler links them."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "interleave_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if _links_sanitized(cxx, tmp_path) \
        else []
    print("sanitizers:", "address,undefined" if san else "not linked by this compiler")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", os.path.join(PKG_DIR, "csrc"),
                    os.path.join(ROOT, "tools", "interleave_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "interleave_host_check: OK" in r.stdout, r.stdout + r.stderr


# ------------------------------------------------ the restatement's identities
def test_restatement_identities():
    import channel_ref
    import interleave_ref
    import ratematch_ref
    from test_gpu_channel import _graph_h
    count, frame0, p = 3, 1000, 3
    cases = ((hstd_for("wimax_576_0.5"), False, RM_W576, 576),
             (_graph_h("tiny66")[0], False, RateMatch((0, 7, 45, 46, 47, 65), (1, 33, 44)), 66))
    for H, ira, rm, n in cases:
        u, c = ratematch_ref.bits(H, ira, rm, SEED, p, frame0, count)
        E = rm.n_transmitted(n)
        for spec in (ChannelSpec("rayleigh", "bpsk"), ChannelSpec("rayleigh", "qam16", "exact"),
                     ChannelSpec("awgn", "qam64", "maxlog"), ChannelSpec("rayleigh", "qpsk")):
            if E % spec.bps:
                continue
            sigma = 0.3
            want, Mw = ratematch_ref.frames_llr(spec, rm, c, SEED, p, sigma, frame0)
            # no interleaver, the identity, block_len 1: ratematch_ref exactly
            for perm in (None, il.identity(E).perm):
                got, M = interleave_ref.frames_llr(spec, rm, perm, 1, c, SEED, p, sigma, frame0)
                np.testing.assert_array_equal(got, want)
                np.testing.assert_array_equal(M, Mw)
            # a permutation moves LLRs (the noise of position t now lands on another column) ...
            perm = il.random(E, 7).perm
            got, _ = interleave_ref.frames_llr(spec, rm, perm, 1, c, SEED, p, sigma, frame0)
            tx = rm.transmitted(n)
            assert not np.array_equal(got, want) and np.isfinite(got).all()
            np.testing.assert_array_equal(got[:, list(rm.punctured)], 0.0)
            np.testing.assert_array_equal(got[:, list(rm.shortened)], -1.0e4)
            # ... but not the bits: at a vanishing sigma every transmitted column carries its codeword sign
            quiet, _ = interleave_ref.frames_llr(spec, rm, perm, 3, c, SEED, p, 1e-4, frame0)
            np.testing.assert_array_equal(quiet[:, tx] > 0, c[:, tx] == 1)
            if spec.model != "rayleigh":
                # AWGN has no fade to share
                np.testing.assert_array_equal(
                    interleave_ref.frames_llr(spec, rm, perm, 5, c, SEED, p, sigma, frame0)[0], got)
    # columns(): the header's example and a pattern plus a permutation
    assert interleave_ref.columns(None, (0, 3, 1, 4, 2, 5), 6).tolist() == [0, 3, 1, 4, 2, 5]
    assert interleave_ref.columns(RateMatch((0, 7), (3,)), (6, 0, 3, 1, 5, 2, 4), 10).tolist() == [9, 1, 5, 2, 8, 4, 6]
    assert interleave_ref.columns(RateMatch((0, 7), (3,)), None, 10).tolist() == [1, 2, 4, 5, 6, 8, 9]
    # block fading: index floor(s / L) of the existing draw; a ragged last block; L >= S: one fade per frame
    for F in (1000, 1001):
        h = channel_ref.fades(SEED, F, p, 144)
        np.testing.assert_array_equal(interleave_ref.block_fades(SEED, F, p, 144, 1), h)
        b5 = interleave_ref.block_fades(SEED, F, p, 144, 5)
        assert len(b5) == 144 and len(np.unique(b5)) == 29
        np.testing.assert_array_equal(b5[::5], h[:29])
        np.testing.assert_array_equal(b5[140:], np.full(4, h[28]))  # the ragged last block
        assert b5[4] == h[0] and b5[5] == h[1] and b5[9] == h[1]     # odd index 1: the draw's second uniform
        for L in (144, 145, 10 ** 6):
            one = interleave_ref.block_fades(SEED, F, p, 144, L)
            assert len(one) == 144 and len(np.unique(one)) == 1 and one[0] == h[0]
    assert channel_ref.fades(SEED, 1000, p, 1)[0] != channel_ref.fades(SEED, 1001, p, 1)[0]
