"""HARQ plans without a GPU: the plan builders and the command line's grammar
(ldpc_amd/harq.py), the restatement's identities (tests/harq_ref.py),
simulate_harq's formulas and refusals, the command line, the header and the
library's argument checks.
"""
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
from ldpc_amd import harq
from ldpc_amd import interleave as il
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec
from ldpc_amd.harq import HarqPlan
from ldpc_amd.ratematch import RateMatch

SEED = 20260213
NEW = ("ldpc_harq_set", "ldpc_harq_get")


# ------------------------------------------------------------ the builders
def test_circular_buffer_hand_values():
    # n = 10, no shortening: IR windows of 4 at offsets 0, 4, 8 (a wrap)
    p = HarqPlan.ir(10, 3, 4)
    assert p.tx == ((0, 1, 2, 3), (4, 5, 6, 7), (8, 9, 0, 1))
    assert (p.R, len(p), p.lengths, p.n_sent(2), p.kind) == (3, 3, (4, 4, 4), 4, "ir")
    assert p.info() == {"kind": "ir", "R": 3, "E": [4, 4, 4], "step": 4, "buffer": 10}
    # Chase: step = 0, the same columns again; E = None sends the whole buffer
    c = HarqPlan.chase(10, 2, 6)
    assert c.tx == ((0, 1, 2, 3, 4, 5),) * 2 and c.kind == "chase" and c.info()["step"] == 0
    assert HarqPlan.chase(10, 3).tx == (tuple(range(10)),) * 3
    # shortened columns are not in the buffer: N = 8, and the whole-buffer Chase skips them
    s = HarqPlan.circular(10, 3, 5, 3, shortened=(1, 4))
    assert s.tx == ((0, 2, 3, 5, 6), (5, 6, 7, 8, 9), (8, 9, 0, 2, 3))
    assert HarqPlan.chase(10, 2, shortened=(1, 4)).tx == ((0, 2, 3, 5, 6, 7, 8, 9),) * 2
    # an order of the buffer's own
    o = HarqPlan.ir(6, 2, 4, order=(5, 3, 1, 0, 2, 4))
    assert o.tx == ((5, 3, 1, 0), (2, 4, 5, 3))
    # the module's worked example: offsets 0, 384, 192 on 576 columns
    w = HarqPlan.ir(576, 3, 384)
    assert [t[0] for t in w.tx] == [0, 384, 192] and w.tx[1][191:193] == (575, 0)
    counts = np.bincount(np.concatenate(w.tx), minlength=576)
    assert (counts == 2).all()
    # truncated: the first R' transmissions, immutable
    assert w.truncated(2).tx == w.tx[:2] and w.truncated(3) == w and w.truncated(1).R == 1
    with pytest.raises(Exception):
        w.tx = ()
    assert HarqPlan.from_lists([[3, 1], [2]]).tx == ((3, 1), (2,))
    assert HarqPlan.from_lists([[3, 1], [2]]) == HarqPlan(((3, 1), (2,)))


def test_builders_refuse():
    for call, msg in ((lambda: HarqPlan.circular(10, 2, 11, 0), "E = 11 > N = 10"),
                      (lambda: HarqPlan.ir(10, 2, 9, shortened=(0, 1)), "E = 9 > N = 8"),
                      (lambda: HarqPlan.chase(10, 0), "transmissions"),
                      (lambda: HarqPlan.chase(10, 9), "transmissions"),
                      (lambda: HarqPlan.ir(10, 2, 0), "E >= 1"),
                      (lambda: HarqPlan.circular(10, 2, 4, -1), "step"),
                      (lambda: HarqPlan.ir(6, 2, 4, order=(0, 1, 2, 3, 4, 4)), "order"),
                      (lambda: HarqPlan.ir(6, 2, 4, shortened=(0,), order=(0, 1, 2, 3, 4, 5)), "order"),
                      (lambda: HarqPlan(()), "transmissions"),
                      (lambda: HarqPlan(((0, 1),) * 9), "transmissions"),
                      (lambda: HarqPlan(((0, 1), ())), "sends nothing"),
                      (lambda: HarqPlan(((0, 1, 1),)), "twice"),
                      (lambda: HarqPlan(((0, -1),)), "negative"),
                      (lambda: HarqPlan(((0, 1.5),)), "integers"),
                      (lambda: HarqPlan("01"), "column lists"),
                      (lambda: HarqPlan(((0, 1),)).truncated(2), "truncated"),
                      (lambda: HarqPlan(((0, 1),)).truncated(0), "truncated"),
                      (lambda: HarqPlan(((0, 10),)).validate(10), "outside"),
                      (lambda: HarqPlan(((0, 3),)).validate(10, shortened=(3,)), "shortens"),
                      (lambda: HarqPlan(((0, 3, 4),)).validate(10, bps=2), "multiple of bps")):
        with pytest.raises(ValueError, match=msg):
            call()
    # the same column in two transmissions is the point of a plan
    assert HarqPlan(((0, 1), (1, 0))).validate(2, bps=2).R == 2


def test_parse_accept_reject_table(tmp_path):
    assert harq.parse("chase:3", 576) == HarqPlan.chase(576, 3)
    assert harq.parse(" Chase:2:384 ", 576) == HarqPlan.chase(576, 2, 384)
    assert harq.parse("ir:3:1152", 2304) == HarqPlan.ir(2304, 3, 1152)
    assert harq.parse("ir:2:8", 20, shortened=(0, 1)).tx[0] == tuple(range(2, 10))
    assert HarqPlan.parse("ir:2:4", 10) == HarqPlan.ir(10, 2, 4)
    path = tmp_path / "plan.txt"
    path.write_text("0 1 2 3\n\n7 6 5 4\n")
    f = harq.parse(f"file:{path}", 10)
    assert f.tx == ((0, 1, 2, 3), (7, 6, 5, 4)) and f.kind == "file"
    with pytest.raises(ValueError, match="outside"):
        harq.parse(f"file:{path}", 7)
    with pytest.raises(ValueError, match="shortens"):
        harq.parse(f"file:{path}", 10, shortened=(5,))
    with pytest.raises(OSError):
        harq.parse(f"file:{tmp_path}/missing", 10)
    (tmp_path / "bad.txt").write_text("0 x\n")
    with pytest.raises(ValueError, match="integers"):
        harq.parse(f"file:{tmp_path}/bad.txt", 10)
    (tmp_path / "empty.txt").write_text("\n")
    with pytest.raises(ValueError, match="no transmissions"):
        harq.parse(f"file:{tmp_path}/empty.txt", 10)
    for bad in ("", "chase", "ir:3", "ir:3:4:5", "chase:1:2:3", "arq:2", "chase:x", "ir:2:1.5", "file:", "none"):
        with pytest.raises(ValueError):
            harq.parse(bad, 10)
    with pytest.raises(ValueError, match="E = 11"):
        harq.parse("ir:2:11", 10)
    with pytest.raises(ValueError):
        harq.split_spec(3)
    assert harq.resolve(HarqPlan.ir(10, 2, 4), 10) == harq.resolve("ir:2:4", 10)
    with pytest.raises(ValueError, match="HarqPlan"):
        harq.resolve(((0, 1),), 10)


# ------------------------------------------------------------ the restatement
def test_seed_wraps_at_two_to_the_64():
    import harq_ref
    step = 0x9E3779B97F4A7C15
    assert harq.tx_seed(SEED, 0) == SEED == harq_ref.tx_seed(SEED, 0)
    assert harq.tx_seed(SEED, 1) == SEED + step
    assert harq.tx_seed(SEED, 2) == (SEED + 2 * step) % 2 ** 64 != SEED + 2 * step   # 2 step > 2^64
    assert harq.tx_seed(2 ** 64 - 1, 1) == step - 1
    for r in range(8):
        assert harq.tx_seed(SEED, r) == harq_ref.tx_seed(SEED, r) < 2 ** 64
    assert len({harq.tx_seed(SEED, r) for r in range(8)}) == 8


def test_restatement_identities():
    """A one-transmission plan tx[pi] is interleave_ref.frames_llr exactly; a
    second transmission adds its own LLRs, exactly, to the columns it carries."""
    import harq_ref
    import interleave_ref
    import ratematch_ref
    from test_gpu_channel import _graph_h
    count, frame0, p, sigma = 3, 1000, 3, 0.3
    rm_w = RateMatch(tuple(288 + 6 * i for i in range(48)), tuple(range(24)))
    cases = ((hstd_for("wimax_576_0.5"), rm_w, 576), (_graph_h("tiny66")[0], RateMatch((0, 7, 45, 46, 47, 65), (1, 33, 44)), 66))
    for H, rm, n in cases:
        u, c = ratematch_ref.bits(H, False, rm, SEED, p, frame0, count)
        E = rm.n_transmitted(n)
        perm = il.random(E, 7).perm
        col = interleave_ref.columns(rm, perm, n)
        for spec, bl in ((ChannelSpec("rayleigh", "bpsk"), 3), (ChannelSpec("rayleigh", "qam16", "exact"), 1),
                         (ChannelSpec("awgn", "qam64", "maxlog"), 1)):
            if E % spec.bps:
                continue
            want, M = interleave_ref.frames_llr(spec, rm, perm, bl, c, SEED, p, sigma, frame0)
            got, bound = harq_ref.frames_llr(spec, [col], rm.shortened, bl, c, SEED, p, sigma, frame0)
            np.testing.assert_array_equal(got, want)  # -0.0 == +0.0
            assert not np.signbit(got[:, list(rm.punctured)]).any()
            np.testing.assert_array_equal(bound[:, col], 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want[:, col]))
            assert (bound[:, list(rm.punctured) + list(rm.shortened)] == 0.0).all()
            # a second transmission of the first half: those columns gain transmission 1's LLRs, the rest stay
            half = col[:(E // 2) // spec.bps * spec.bps]
            two, b2 = harq_ref.frames_llr(spec, [col, half], rm.shortened, bl, c, SEED, p, sigma, frame0)
            rest = np.setdiff1d(np.arange(n), half)
            np.testing.assert_array_equal(two[:, rest], got[:, rest])
            for f in range(count):
                sent, _ = interleave_ref.sent_llr(spec, c[f, half], harq_ref.tx_seed(SEED, 1), frame0 + f, p, sigma, bl)
                np.testing.assert_array_equal(two[f, half], got[f, half] + sent)
            assert (b2[:, half] > bound[:, half]).all()
            # the second transmission is another realisation: it differs from a repeat of the first
            assert not np.array_equal(two[:, half], 2.0 * got[:, half])
            # no noise to speak of: every sent column carries its codeword sign
            quiet, _ = harq_ref.frames_llr(spec, [col, half], rm.shortened, bl, c, SEED, p, 1e-4, frame0)
            np.testing.assert_array_equal(quiet[:, col] > 0, c[:, col] == 1)


# ------------------------------------------------------------ simulate_harq
def test_harq_point_formulas_on_made_up_counters():
    # 1000 frames; 400, 100, 10 fail after 1, 2, 3 transmissions of 100, 60, 40 positions; k_info = 50, 16-QAM
    ctr = np.array([[1000, 400, 3000, 0, 600, 0, 12000],
                    [1000, 100, 500, 0, 900, 0, 8000],
                    [1000, 10, 40, 0, 990, 0, 5000]], np.int64)
    pt = mc.harq_point(ctr, (100, 60, 40), 50, 4)
    assert pt["fer_after"] == [0.4, 0.1, 0.01]
    assert pt["ber_after"] == [3000 / 50000, 500 / 50000, 40 / 50000]
    assert pt["avg_iterations"] == [12.0, 8.0, 5.0]
    assert pt["p_tx"] == [1.0, 0.4, 0.1]
    assert pt["avg_tx"] == pytest.approx(1.5, abs=1e-15)
    assert pt["bits_sent"] == pytest.approx(100 + 0.4 * 60 + 0.1 * 40, abs=1e-12)
    assert pt["throughput"] == pytest.approx(50 * 0.99 / (128.0 / 4), rel=1e-15)
    # one transmission: the plain rate times (1 - FER)
    one = mc.harq_point(ctr[:1], (100,), 50, 1)
    assert one["p_tx"] == [1.0] and one["avg_tx"] == 1.0 and one["bits_sent"] == 100.0
    assert one["throughput"] == pytest.approx(0.5 * 0.6, rel=1e-15)
    with pytest.raises(ValueError):
        mc.harq_point(ctr, (100, 60), 50, 4)
    assert "nested" in mc.harq_point.__doc__ and "nested" in mc.simulate_harq.__doc__


def test_simulate_harq_refuses_before_any_device_call(monkeypatch):
    qam = ChannelSpec("awgn", "qam16")
    plan = HarqPlan.chase(576, 2)
    for kw, msg in ((dict(mode="parity", channel=qam), "physical"),
                    (dict(), "channel model"),
                    (dict(channel=ChannelSpec()), "channel model"),
                    (dict(channel=qam, interleaver="regular"), "interleaver"),
                    (dict(channel=qam, interleaver=il.regular(576)), "interleaver"),
                    (dict(channel=qam, rate_match=RateMatch((300, 301, 302, 303), ())), "puncturing"),
                    (dict(channel=qam, rate_match=RateMatch((300, 301, 302, 303), (0, 1, 2, 3))), "puncturing"),
                    (dict(channel=qam, fading_block=4), "Rayleigh")):
        with pytest.raises(ValueError, match=msg):
            mc.simulate_harq(None, [0.0], 1, 5, plan, **kw)
    for bad in ("chase", "foo:2", ((0, 1),), None):
        with pytest.raises(ValueError):
            mc.simulate_harq(None, [0.0], 1, 5, bad, channel=qam)
    from ldpc_amd import device

    def no_graph(*a, **k):
        raise AssertionError("simulate_harq() made a graph before it checked the plan")
    monkeypatch.setattr(device, "Graph", no_graph)
    W = "wimax_576_0.5"
    for kw, msg in ((dict(harq="ir:2:577"), "E = 577"),
                    (dict(harq="ir:2:386"), "multiple of bps"),
                    (dict(harq=HarqPlan(((0, 1, 2, 600),))), "outside"),
                    (dict(harq=HarqPlan(((0, 1, 2, 3),)), rate_match=RateMatch((), (3,))), "shortens")):
        with pytest.raises(ValueError, match=msg):
            mc.simulate_harq(W, [0.0], 1, 5, channel=qam, **kw)
    for kw in (dict(harq="chase:2"), dict(harq="ir:3:384"), dict(harq="ir:2:384", rate_match=RateMatch((), (0, 1, 2, 3))),
               dict(harq=plan, interleaver="none")):
        with pytest.raises(AssertionError, match="made a graph"):
            mc.simulate_harq(W, [0.0], 1, 5, channel=qam, **kw)


# ------------------------------------------------------------ the command line
def test_cli_accept_reject_table(capsys):
    head = ["--matrix", "wimax_576_0.5"]
    phys = ["--mode", "physical"]
    qam = phys + ["--channel", "awgn", "--modulation", "qam16"]
    ray = phys + ["--channel", "rayleigh", "--fading-block", "24"]
    assert mc.parse_args(head).harq is None and mc.parse_args(head).harq_json is None
    a = mc.parse_args(head + qam + ["--harq", "ir:3:384", "--harq-json", "out.json"])
    assert (a.harq, a.harq_json) == ("ir:3:384", "out.json")
    assert mc.parse_args(head + ray + ["--harq", "chase:4"]).harq == "chase:4"
    assert mc.parse_args(head + qam + ["--harq", "chase:2", "--shorten", "0:24"]).shorten == "0:24"
    assert mc.parse_args(head + qam + ["--harq", "chase:2", "--interleaver", "none"]).interleaver is None
    assert mc.parse_args(head + qam + ["--harq", "file:plan.txt", "--cn-rule", "nms", "--schedule", "layered"]).harq
    for argv in (["--harq", "chase:2"],                                          # parity mode
                 phys + ["--harq", "chase:2"],                                   # no channel model
                 phys + ["--channel", "reference", "--harq", "chase:2"],
                 qam + ["--harq", "chase:2", "--interleaver", "regular"],        # an interleaver
                 qam + ["--harq", "chase:2", "--puncture", "k:n:6"],             # a puncturing pattern
                 qam + ["--harq-json", "out.json"],                              # --harq-json alone
                 qam + ["--harq", "chase"], qam + ["--harq", "arq:2"], qam + ["--harq", "ir:2"],
                 qam + ["--harq", "chase:2", "--output-json", "x.json"],
                 qam + ["--harq", "chase:2", "--stats-json", "x.json"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def test_cli_refuses_a_plan_the_code_cannot_carry(monkeypatch, capsys):
    def no_simulate(*a, **k):
        raise AssertionError("main() reached simulate_harq() with a plan it should have refused")
    monkeypatch.setattr(mc, "simulate_harq", no_simulate)
    base = ["--matrix", "wimax_576_0.5", "--mode", "physical", "--channel", "awgn", "--modulation", "qam16"]
    with pytest.raises(SystemExit, match="E = 577"):
        mc.main(base + ["--harq", "ir:2:577"])
    with pytest.raises(SystemExit, match="multiple of bps"):
        mc.main(base + ["--harq", "ir:2:386"])
    with pytest.raises(SystemExit, match="--harq"):
        mc.main(base + ["--harq", "file:/nonexistent/plan"])
    with pytest.raises(AssertionError, match="reached simulate_harq"):
        mc.main(base + ["--harq", "ir:3:384"])


def test_header_line_and_json(tmp_path):
    plan = HarqPlan.ir(576, 3, 384)
    head = mc.harq_header(plan.info())
    assert head == "HARQ ir  R 3  E_r 384 384 384  step 384"
    assert mc.harq_header(HarqPlan(((0, 1), (2,))).info()) == "HARQ custom  R 2  E_r 2 1"
    ctr = np.arange(3 * 1 * 7, dtype=np.int64).reshape(3, 1, 7) + 1
    res = {"plan": plan.info(), "sigma": [0.5], "counters": ctr,
           "points": [{"snr_db": 2.0, "frames": 1, **mc.harq_point(ctr[:, 0], plan.lengths, 288, 4)}]}
    mc.harq_to_json(str(tmp_path / "h.json"), 7, res)
    doc = json.loads((tmp_path / "h.json").read_text())
    assert doc["seed"] == 7 and doc["plan"]["R"] == 3 and doc["counters"] == ctr.tolist()
    assert set(doc["points"][0]) >= {"fer_after", "ber_after", "avg_iterations", "p_tx", "avg_tx", "bits_sent",
                                     "throughput"}


# ------------------------------------------------------------ the library
def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert re.search(r"^#define\s+LDPC_HARQ_MAX_TX\s+8\b", txt, flags=re.M) and harq.MAX_TX == 8
    assert "0x9E3779B97F4A7C15" in txt
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5


_NULL_CALLS = r"""
import ctypes, os
from ldpc_amd import _lib
L = _lib.lib()
lens = (ctypes.c_int32 * 2)(2, 1)
cols = (ctypes.c_int32 * 3)(0, 1, 1)
out = (ctypes.c_int32 * 8)(*([77] * 8))
n = ctypes.c_int32(77)
calls = [("set NULL decoder", lambda: L.ldpc_harq_set(None, 2, lens, cols)),
         ("set NULL decoder, clearing", lambda: L.ldpc_harq_set(None, 0, None, None)),
         ("set NULL decoder, bad count", lambda: L.ldpc_harq_set(None, 9, lens, cols)),
         ("set NULL decoder, NULL lists", lambda: L.ldpc_harq_set(None, 2, None, None)),
         ("get NULL decoder", lambda: L.ldpc_harq_get(None, ctypes.byref(n), out, None, 0)),
         ("get NULL decoder, NULL n_tx", lambda: L.ldpc_harq_get(None, None, None, cols, 3))]
for what, call in calls:
    rc = call()
    assert rc == _lib.LDPC_EINVAL == -22, (what, rc)
    assert b"NULL decoder" in L.ldpc_last_error(), (what, L.ldpc_last_error())
assert n.value == 77 and list(out) == [77] * 8 and list(cols) == [0, 1, 1]
assert not _lib.hip_started_here()
opened = [os.readlink(f"/proc/self/fd/{fd}") for fd in os.listdir("/proc/self/fd")
          if os.path.exists(f"/proc/self/fd/{fd}")]
assert not [p for p in opened if p.startswith("/dev/kfd") or p.startswith("/dev/dri")], opened
print("ok")
"""


def test_argument_checks_touch_no_device():
    """ldpc_harq_set(None, ...) is -22, in a process of its own: nothing else in it can have started the runtime."""
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
    """csrc/rate_match_host.h's harq_validate (what ldpc_harq_set validates
    with) in tools/harq_host_check.cpp, a program of its own: built with -Wall
    -Wextra -Werror, and under the address and undefined-behaviour sanitizers
    where the host compiler links them."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++") or "/opt/rocm/llvm/bin/clang++"
    exe = str(tmp_path / "harq_host_check")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if _links_sanitized(cxx, tmp_path) \
        else []
    print("sanitizers:", "address,undefined" if san else "not linked by this compiler")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *san, "-I", os.path.join(PKG_DIR, "csrc"),
                    os.path.join(ROOT, "tools", "harq_host_check.cpp"), "-o", exe], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "harq_host_check: OK" in r.stdout, r.stdout + r.stderr
