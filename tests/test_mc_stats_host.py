"""Host side of the physical-mode Monte-Carlo statistics (ldpc_mc_stats_enable /
ldpc_mc_stats_read): the header and the symbol list, the argument checks that
need no device, fer_by_max_iter, the multi-rank reduction, the command line and
the --stats-json writer.  No GPU."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mc_stats_ref
from conftest import PKG_DIR, ROOT
from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc

NEW = ("ldpc_mc_stats_enable", "ldpc_mc_stats_read")


def test_header_symbols_and_abi_version():
    txt = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    for name in NEW:
        assert re.search(rf"^int\s+{name}\s*\(", txt, flags=re.M), name
        assert name in _lib.EXPORTED
        assert hasattr(_lib.lib(), name)
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.lib().ldpc_abi_version() == 5


_NULL_CALLS = r"""
import os, sys
import numpy as np
from ldpc_amd import _lib
L = _lib.lib()
h, u, f, nf = np.zeros(6, np.int64), np.zeros(2, np.int64), np.zeros((4, 2), np.int64), np.zeros(2, np.int64)
calls = [("enable NULL", lambda: L.ldpc_mc_stats_enable(None, 1, 0), b"NULL decoder"),
         ("enable max_failed < 0", lambda: L.ldpc_mc_stats_enable(None, 1, -1), b"max_failed"),
         ("read NULL", lambda: L.ldpc_mc_stats_read(None, 0, _lib.ptr(h), 6, _lib.ptr(u), _lib.ptr(f), 4, _lib.ptr(nf)),
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


def test_null_decoder_and_negative_max_failed_touch_no_device():
    """In a process of its own: nothing else in it can have started the runtime."""
    env = dict(os.environ, PYTHONPATH=PKG_DIR + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-c", _NULL_CALLS], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_fer_by_max_iter():
    hist = np.array([0, 10, 30, 0, 20, 40])  # T = 5: 60 of 100 converge, at iterations 1, 2, 4
    np.testing.assert_array_equal(mc.fer_by_max_iter(hist), [1.0, 0.9, 0.6, 0.6, 0.4])
    out = mc.fer_by_max_iter(hist)
    assert out.dtype == np.float64 and out.shape == (5,)
    assert out[-1] == hist[5] / hist.sum()  # the run's own detected FER
    np.testing.assert_array_equal(mc.fer_by_max_iter([0, 0, 0, 7]), [1.0, 1.0, 1.0])  # every frame failed
    np.testing.assert_array_equal(mc.fer_by_max_iter([0, 0, 0, 0]), [0.0, 0.0, 0.0])  # an empty run
    np.testing.assert_array_equal(mc.fer_by_max_iter([5, 0]), [0.0])                  # T = 1


def test_simulate_refuses_before_any_device_call():
    """matrix=None: simulate() raises before it loads a code or makes a graph."""
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, stats=True)
    with pytest.raises(ValueError, match="physical"):
        mc.simulate(None, [0.0], 1, 5, mode="parity", stats=True, max_failed=4)
    with pytest.raises(ValueError, match="ranks"):
        mc.simulate(None, [0.0], 4, 5, mode="physical", cn_rule="nms", stats=True, max_failed=4, world=2,
                    allreduce=lambda a: a)
    with pytest.raises(ValueError, match="max_failed"):
        mc.simulate(None, [0.0], 1, 5, mode="physical", stats=True, max_failed=-1)


def test_cli_rules(capsys):
    head = ["--matrix", "x"]
    a = mc.parse_args(head + ["--mode", "physical", "--cn-rule", "nms", "--stats-json", "s.json", "--max-failed", "64"])
    assert (a.stats_json, a.max_failed) == ("s.json", 64)
    a = mc.parse_args(head + ["--mode", "physical", "--stats-json", "s.json"])
    assert (a.stats_json, a.max_failed) == ("s.json", 0)
    a = mc.parse_args(head)
    assert (a.stats_json, a.max_failed) == (None, 0)
    for argv in (["--stats-json", "s.json"],                                       # no --mode physical
                 ["--mode", "parity", "--stats-json", "s.json"],
                 ["--mode", "parity", "--stats-json", "s.json", "--max-failed", "4"],
                 ["--max-failed", "4"],
                 ["--mode", "physical", "--max-failed", "4"],                      # no --stats-json
                 ["--mode", "physical", "--stats-json", "s.json", "--max-failed", "-1"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()


def _fake_run(T=6, B=40, points=2):
    """Per-frame results of a made-up run -> (counters [points, 7], stats dicts)."""
    rng = np.random.default_rng(5)
    ctr, stats = [], []
    for p in range(points):
        conv = rng.integers(-1, T, B)
        status = (conv < 0).astype(np.int32)
        u = rng.integers(0, 2, (B, 4)).astype(np.uint8)
        z = np.concatenate([u ^ 1, np.ones((B, 3), np.uint8)], axis=1)
        z[status != 0, 0] ^= 1       # a failed frame has one info-bit error
        z[(conv == 2), 1] ^= 1       # the frames converging at iteration 2 are undetected errors
        o = {"z": z, "conv": conv, "status": status}
        iters = np.where(conv >= 0, conv + 1, T)
        k = u.shape[1]
        err = np.where(status != 0, ((z[:, :k] ^ 1) != u).sum(axis=1), 0)
        ctr.append([B, int(status.sum()), int(err.sum()), int(conv[conv >= 0].sum()), int((conv >= 0).sum()), 0,
                    int(iters.sum())])
        stats.append(mc_stats_ref.stats(u, o, T))
    return np.array(ctr, np.int64), stats


def test_multi_rank_reduction_doubles():
    """run_sweep with stand-ins for the device and an allreduce that doubles:
    counters, hist and the undetected totals double, and the identities hold."""
    T, snrs = 6, [-1.0, 0.5]
    ctr, stats = _fake_run(T)
    assert all(st["undetected_frames"] > 0 for st in stats)
    # max_failed = 0 on every rank: the device keeps no record and reports every failure as dropped
    local = [dict(st, failed=np.zeros((0, 2), np.int64), failed_dropped=int(st["hist"][T])) for st in stats]
    assert all(st["failed_dropped"] > 0 for st in local)
    calls = []

    def allreduce(a):
        calls.append(a.dtype)
        return 2 * a
    got_ctr, got = mc.run_sweep(None, snrs, 80, T, rank=1, world=2, allreduce=allreduce,
                                counter_fn=lambda sig, cnt, f0: ctr, stats_fn=lambda p: local[p])
    assert calls == [np.dtype(np.int64)] * 2
    np.testing.assert_array_equal(got_ctr, 2 * ctr)
    for p, st in enumerate(got):
        np.testing.assert_array_equal(st["hist"], 2 * stats[p]["hist"])
        assert st["hist"].dtype == np.int64
        assert st["undetected_frames"] == 2 * stats[p]["undetected_frames"]
        assert st["undetected_bit_errors"] == 2 * stats[p]["undetected_bit_errors"]
        assert len(st["failed"]) == 0 and st["failed_dropped"] == 2 * local[p]["failed_dropped"] == st["hist"][T]
        mc_stats_ref.assert_identities(st["hist"], got_ctr[p])
        assert (st["snr_db"], st["frames"]) == (snrs[p], 80)
        np.testing.assert_array_equal(st["fer_by_max_iter"], mc.fer_by_max_iter(st["hist"]))
        assert st["fer_by_max_iter"][-1] == got_ctr[p][1] / got_ctr[p][0]
    # one rank: nothing is reduced, the list passes through; without stats_fn the old return value
    one_ctr, one = mc.run_sweep(None, snrs, 40, T, counter_fn=lambda sig, cnt, f0: ctr, stats_fn=lambda p: stats[p])
    for p, st in enumerate(one):
        mc_stats_ref.assert_equal(st, stats[p], f"point {p}")
        mc_stats_ref.assert_identities(st["hist"], one_ctr[p])
    assert isinstance(mc.run_sweep(None, snrs, 40, T, counter_fn=lambda sig, cnt, f0: ctr), np.ndarray)
    # failure lists cannot be reduced
    with pytest.raises(ValueError, match="ranks"):
        mc.run_sweep(None, snrs, 80, T, world=2, allreduce=allreduce, counter_fn=lambda sig, cnt, f0: ctr,
                     stats_fn=lambda p: stats[p])
    with pytest.raises(ValueError, match="allreduce"):
        mc.reduce_stats(local, snrs, world=2)


def test_stats_json_writer(tmp_path):
    T, snrs = 6, [-1.0, 0.5]
    ctr, stats = _fake_run(T)
    pts = mc.reduce_stats(stats, snrs)
    path = tmp_path / "stats.json"
    mc.stats_to_json(str(path), 1234, pts)
    doc = json.loads(path.read_text())
    assert doc["seed"] == 1234 and len(doc["points"]) == 2
    for p, d in enumerate(doc["points"]):
        assert set(d) == {"snr_db", "frames", "hist", "fer_by_max_iter", "undetected_frames",
                          "undetected_bit_errors", "failed", "failed_dropped"}
        assert len(d["hist"]) == T + 1 and len(d["fer_by_max_iter"]) == T
        assert d["hist"] == stats[p]["hist"].tolist() and d["frames"] == 40 and d["snr_db"] == snrs[p]
        assert d["failed"] == stats[p]["failed"].tolist() and len(d["failed"]) == ctr[p][1]
        assert d["undetected_frames"] == stats[p]["undetected_frames"] > 0
        assert d["fer_by_max_iter"][-1] == ctr[p][1] / ctr[p][0]
    assert json.loads(json.dumps(doc)) == doc
