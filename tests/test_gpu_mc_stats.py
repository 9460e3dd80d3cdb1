"""Physical-mode Monte-Carlo statistics on the GPU (ldpc_mc_stats_enable /
ldpc_mc_stats_read): the histogram of the convergence iteration, the
undetected errors and the failed-frame records of every Monte-Carlo path.

Expected values are the CPU restatement (tests/mc_stats_ref.py on
minsum_ref / qminsum_ref) of the frames Decoder.generate returns -- the method
of test_monte_carlo_counters_equal_restatement -- so every comparison is
EQUALITY.  The sum-product decoder has no bit-exact restatement; it is held to
the same GPU's phys_decode of the generated frames (the same kernel on the same
-(float)llr inputs)."""
import functools
import json

import numpy as np
import pytest

import ldpc_amd
import mc_stats_ref as ref
import minsum_ref
import qminsum_ref
from ldpc_amd import _lib, ira
from ldpc_amd import montecarlo as mc

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA = 0.75
B, T = 256, 20
Q = dict(qbits=6, llr_scale=4.0)


# ------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module", autouse=True)
def _release():
    """The decoders and expected values live for this module only."""
    yield
    for key in list(_DECODERS):
        _DECODERS.pop(key).close()
    for cached in (_setup, _frames, _want):
        cached.cache_clear()


_DECODERS = {}


@functools.lru_cache(maxsize=None)
def _setup(code, cap=B):
    """(frame-source decoder, physical graph, H of the physical graph)"""
    from ldpc_amd.device import Decoder, Graph
    if code == "ira":
        H = ira.small_ira_matrix()
        g = Graph.cached(H)
        _DECODERS[code, cap] = Decoder(g, cap)
        return _DECODERS[code, cap], g, H
    edd = ldpc_amd.load_committed_code(code)
    H = edd.physical_matrix()
    _DECODERS[code, cap] = Decoder(Graph.cached(edd._h_std), cap)
    return _DECODERS[code, cap], Graph.cached(H), H


@functools.lru_cache(maxsize=None)
def _frames(code, snrs, frame0=0, count=B, cap=B):
    dec = _setup(code, cap)[0]
    out = []
    for p, s in enumerate(snrs):
        parts = [dec.generate(SEED, p, mc.sigma_for_snr(s), frame0 + i, min(cap, count - i))
                 for i in range(0, count, cap)]  # generate() takes up to the decoder's capacity
        u, llr = (np.concatenate([q[i] for q in parts]) for i in range(2))
        u.setflags(write=False)
        llr.setflags(write=False)
        out.append((u, llr))
    return out


@functools.lru_cache(maxsize=None)
def _want(code, snrs, schedule, quant=False, max_iter=T, frame0=0, count=B, cap=B):
    """The restatement's statistics and per-frame results, once per input."""
    H = _setup(code, cap)[2]
    out = []
    for u, llr in _frames(code, snrs, frame0, count, cap):
        if quant:
            o = qminsum_ref.decode(H, llr, max_iter, "nms", schedule, 6, 4.0, 12)
        else:
            o = minsum_ref.decode(H, llr, max_iter, "nms", schedule, ALPHA, 0.5)
        out.append((ref.stats(u, o, max_iter, frame0), o))
    return out


def _run(code, snrs, max_iter=T, frame0=0, count=B, cap=B, stats=True, max_failed=None, **kw):
    """One Monte-Carlo run -> (counters, [statistics per point] or None)."""
    dec, gp, _ = _setup(code, cap)
    sig = [mc.sigma_for_snr(s) for s in snrs]
    dec.mc_stats(stats, (count if max_failed is None else max_failed) if stats else 0)
    try:
        ctr = dec.phys_mc_run(gp, SEED, sig, count, frame0, max_iter, **kw)
        st = [dec.mc_stats_read(p, max_iter) for p in range(len(sig))] if stats else None
    finally:
        dec.mc_stats(False)
    return ctr, st


def _check_run(code, snrs, want, what, **kw):
    """Statistics equal `want`, the identities hold, the counters do not move."""
    ctr, st = _run(code, snrs, **kw)
    off, _ = _run(code, snrs, stats=False, **kw)
    assert np.array_equal(ctr, off), f"{what}: the counters differ with statistics on\n{ctr}\n{off}"
    for p in range(len(snrs)):
        ref.assert_equal(st[p], want[p], f"{what} point {p}")
        ref.assert_identities(st[p]["hist"], ctr[p])
        assert int(st[p]["failed"][:, 1].sum()) == int(ctr[p][2])
    return ctr, st


# ------------------------------------- 1. every path equals the restatement
W576, W576_SNRS = "wimax_576_0.5", (-2.5, 0.0)
# The two points the cases are stated for, and a third, clean one (below)
LDS_SNRS = W576_SNRS + (2.0,)
LDS_PATHS = [("flooding", "phys_reg_kernel", None), ("flooding", "phys_kernel", ("LDPC_PHYS_REG", "0")),
             ("layered", "phys_layered_kernel", None)]


@pytest.mark.parametrize("schedule,kernel,env", LDS_PATHS)
def test_fp32_lds_paths(gpu_available, monkeypatch, schedule, kernel, env):
    """A waterfall point, then clean ones where every frame lands in bin 0 or 1
    (the kernels' hot bins).  At 0 dB that holds for the layered restatement
    (189 + 67 frames); the flooding one puts 72, 170 and 14 frames in bins 0, 1
    and 2 there, so the condition is asserted for every schedule at the third
    point, 2 dB (256 + 0), and at 0 dB for the layered one."""
    from ldpc_amd.device import phys_kernel_name
    want = [w for w, _ in _want(W576, LDS_SNRS, schedule)]
    assert 0 < want[0]["hist"][T] < B
    assert (want[0]["hist"][:T] > 0).sum() >= 5
    assert want[2]["hist"][:2].sum() == B
    if schedule == "layered":
        assert want[1]["hist"][:2].sum() == B
    if env:
        monkeypatch.setenv(*env)
    assert phys_kernel_name(_setup(W576)[1], cn="nms", schedule=schedule) == kernel
    _check_run(W576, LDS_SNRS, want, kernel, cn="nms", schedule=schedule, alpha=ALPHA)


def _compacts(o, count=B):
    """The run compacts: between 1 and count / 4 frames run at one of the host's polls."""
    polls = [it for it in range(T - 1) if it < 4 or (it + 1) % 4 == 0]
    running = [int(((o["conv"] < 0) | (o["conv"] > it)).sum()) for it in polls]
    return any(1 <= r <= count // 4 for r in running)


IRA_SNRS = (-2.5, -2.0)


@pytest.mark.parametrize("schedule,kw", [("flooding", {"hbm": True}), ("layered", {"tile": True})])
def test_fp32_tile_paths(gpu_available, monkeypatch, schedule, kw):
    w = _want("ira", IRA_SNRS, schedule)
    want = [s for s, _ in w]
    assert 0 < want[0]["hist"][T] < B
    assert _compacts(w[1][1])
    _check_run("ira", IRA_SNRS, want, f"tile {schedule}", cn="nms", schedule=schedule, alpha=ALPHA, **kw)
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")
    _check_run("ira", IRA_SNRS, want, f"tile {schedule} without compaction", cn="nms", schedule=schedule,
               alpha=ALPHA, **kw)


# (schedule, SNR pair) of tests/test_gpu_qtile.py::MC_POINTS
Q_POINTS = [("flooding", (-2.5, -2.0)), ("layered", (-1.5, -1.0))]


@pytest.mark.parametrize("schedule,snrs", Q_POINTS)
def test_fixed_point_tile_paths(gpu_available, monkeypatch, schedule, snrs):
    w = _want("ira", snrs, schedule, quant=True)
    want = [s for s, _ in w]
    assert 0 < want[0]["hist"][T] < B
    assert _compacts(w[1][1])
    _check_run("ira", snrs, want, f"qtile {schedule}", cn="nms", schedule=schedule, alpha=ALPHA, qtile=True, **Q)
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")
    _check_run("ira", snrs, want, f"qtile {schedule} without compaction", cn="nms", schedule=schedule, alpha=ALPHA,
               qtile=True, **Q)


# wimax_2304_0.5 has k = 1152 info columns: the count kernels run two blocks per
# tile (one per 1,024 columns), which add their shares of a frame's info-bit
# errors and let the last one bin the tile (mc_stats_tile).  128 frames = two
# tiles; at the second point few enough frames still run at a poll that the run
# compacts into one tile (asserted on the restatement).
W2304, W2304_SNRS, B2 = "wimax_2304_0.5", (-2.5, -2.0), 128
TWO_BLOCKS = [("flooding", {"hbm": True}, False), ("layered", {"tile": True}, False),
              ("flooding", dict(Q, qtile=True), True), ("layered", dict(Q, qtile=True), True)]


@pytest.mark.parametrize("schedule,kw,quant", TWO_BLOCKS)
def test_tile_paths_two_blocks_per_tile(gpu_available, monkeypatch, schedule, kw, quant):
    gp = _setup(W2304, B2)[1]
    assert (gp.n - gp.m + 1023) // 1024 == 2
    w = _want(W2304, W2304_SNRS, schedule, quant=quant, count=B2, cap=B2)
    want = [s for s, _ in w]
    assert 0 < want[0]["hist"][T] < B2
    assert _compacts(w[1][1], B2)
    run = dict(count=B2, cap=B2, cn="nms", schedule=schedule, alpha=ALPHA, **kw)
    _check_run(W2304, W2304_SNRS, want, f"k = 1152 {schedule} {kw}", **run)
    _check_run(W2304, W2304_SNRS, want, f"k = 1152 {schedule} {kw}, again", **run)  # the arrays were left zero
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")
    _check_run(W2304, W2304_SNRS, want, f"k = 1152 {schedule} {kw} without compaction", **run)


# The IRA graph's columns have up to 8 edges, more than phys_quant_reg_kernel's shapes hold, so
# the register kernel runs wimax_576_0.5 (with the scales of MC_POINTS), the generic one both
Q_LDS = [(W576, W576_SNRS, "phys_quant_reg_kernel", None), (W576, W576_SNRS, "phys_quant_kernel", ("LDPC_PHYS_Q_REG", "0")),
         ("ira", Q_POINTS[0][1], "phys_quant_kernel", None)]


@pytest.mark.parametrize("code,snrs,kernel,env", Q_LDS)
def test_fixed_point_lds_paths(gpu_available, monkeypatch, code, snrs, kernel, env):
    from ldpc_amd.device import phys_kernel_name
    want = [s for s, _ in _want(code, snrs, "flooding", quant=True)]
    assert 0 < want[0]["hist"][T] < B
    if env:
        monkeypatch.setenv(*env)
    assert phys_kernel_name(_setup(code)[1], cn="nms", qbits=6) == kernel
    _check_run(code, snrs, want, kernel, cn="nms", alpha=ALPHA, **Q)


def test_fixed_point_lds_layered(gpu_available):
    snrs = Q_POINTS[1][1]
    want = [s for s, _ in _want("ira", snrs, "layered", quant=True)]
    _check_run("ira", snrs, want, "phys_quant_kernel layered", cn="nms", schedule="layered", alpha=ALPHA, **Q)


def test_sum_product_equals_phys_decode(gpu_available):
    """Sum-product flooding (ldpc_phys_mc_run): expected from phys_decode on the generated frames."""
    from ldpc_amd.device import phys_decode
    gp = _setup(W576)[1]
    want = []
    for u, llr in _frames(W576, W576_SNRS):
        o = phys_decode(gp, llr, T)
        want.append(ref.stats(u, o, T))
    assert 0 < want[0]["hist"][T] < B
    _check_run(W576, W576_SNRS, want, "sum-product")


# ---------------------------------------- 2. undetected errors are counted
BCH, BCH_SNRS, BCH_T = "BCH_7_4_1_strip", (-2.0,), 10
BCH_PATHS = [("flooding", {}, False), ("layered", {}, False), ("flooding", {"hbm": True}, False),
             ("layered", {"tile": True}, False), ("flooding", dict(Q), True), ("layered", dict(Q), True),
             ("flooding", dict(Q, qtile=True), True), ("layered", dict(Q, qtile=True), True)]


@pytest.mark.parametrize("schedule,kw,quant", BCH_PATHS)
def test_undetected_errors(gpu_available, schedule, kw, quant):
    """The strip of the (7, 4) code at -2 dB: many frames converge to a codeword
    other than the one sent.  The counters take them for successes; the
    statistics count them."""
    want = [s for s, _ in _want(BCH, BCH_SNRS, schedule, quant=quant, max_iter=BCH_T)]
    assert want[0]["undetected_frames"] >= 5, want[0]
    assert want[0]["undetected_bit_errors"] >= want[0]["undetected_frames"]
    ctr, st = _check_run(BCH, BCH_SNRS, want, f"BCH {schedule} {kw}", max_iter=BCH_T, cn="nms", schedule=schedule,
                         alpha=ALPHA, **kw)
    assert st[0]["undetected_frames"] == want[0]["undetected_frames"]
    assert ctr[0][1] + st[0]["undetected_frames"] <= B  # they are among the counters' successes


# ------------------------------------------------- 3. chunks and frame0
CH = dict(frame0=1000, count=320, cap=128)


@pytest.mark.parametrize("kw", [{}, {"tile": True}])
def test_chunks_and_frame0(gpu_available, kw):
    from ldpc_amd.device import phys_decode
    snrs = (-2.5,)
    want = [s for s, _ in _want(W576, snrs, "layered", **CH)]
    dec, gp, _ = _setup(W576, 128)
    assert dec.capacity == 128  # three chunks: 128, 128, 64
    ctr, st = _check_run(W576, snrs, want, f"chunks {kw}", cn="nms", schedule="layered", alpha=ALPHA, **CH, **kw)
    failed = st[0]["failed"]
    assert len(failed) > 8 and failed[:, 0].min() >= 1000 and failed[:, 0].max() < 1320
    assert (failed[:, 0] >= 1128).any() and (failed[:, 0] >= 1256).any()  # from every chunk
    k = gp.n - gp.m
    for index, errors in failed[:8]:
        u, llr = dec.generate(SEED, 0, mc.sigma_for_snr(snrs[0]), int(index), 1)
        r = phys_decode(gp, llr, T, cn="nms", schedule="layered", alpha=ALPHA, **kw)
        assert r.status[0] != 0, index
        assert int(((r.z[0, :k] ^ 1) != u[0]).sum()) == errors, index


# ----------------------------------------------------------- 4. overflow
@pytest.mark.parametrize("kw", [{}, {"tile": True}])
def test_overflow(gpu_available, kw):
    snrs = (-2.5,)
    want = _want(W576, snrs, "layered", **CH)[0][0]
    ctr, st = _run(W576, snrs, max_failed=8, cn="nms", schedule="layered", alpha=ALPHA, **CH, **kw)
    got = st[0]
    assert len(got["failed"]) == 8 and got["failed_dropped"] == ctr[0][1] - 8 > 0
    assert len(set(got["failed"][:, 0].tolist())) == 8
    assert (np.diff(got["failed"][:, 0]) > 0).all()  # sorted
    by_index = {int(i): int(e) for i, e in want["failed"]}
    for index, errors in got["failed"]:
        assert by_index.get(int(index)) == errors, index
    np.testing.assert_array_equal(got["hist"], want["hist"])
    assert (got["undetected_frames"], got["undetected_bit_errors"]) == \
        (want["undetected_frames"], want["undetected_bit_errors"])
    # max_failed = 0: no list, everything dropped
    ctr0, st0 = _run(W576, snrs, max_failed=0, cn="nms", schedule="layered", alpha=ALPHA, **CH, **kw)
    assert len(st0[0]["failed"]) == 0 and st0[0]["failed_dropped"] == ctr0[0][1]
    np.testing.assert_array_equal(st0[0]["hist"], want["hist"])


# ------------------------------------------------- 5. the prefix property
PREFIX = [(W576, (-2.5,), dict(cn="nms", schedule="layered", alpha=ALPHA)),
          ("ira", (-2.5,), dict(cn="nms", hbm=True, alpha=ALPHA)),
          ("ira", (-2.5,), dict(cn="nms", alpha=ALPHA, **Q))]


@pytest.mark.parametrize("code,snrs,kw", PREFIX)
def test_fer_for_every_smaller_limit(gpu_available, code, snrs, kw):
    """One run at T = 20 gives the FER of a run at any T' <= 20."""
    ctr, st = _run(code, snrs, **kw)
    fer = mc.fer_by_max_iter(st[0]["hist"])
    assert fer[T - 1] == ctr[0][1] / ctr[0][0]
    seen = set()
    for t in (1, 7, 20):
        c, _ = _run(code, snrs, max_iter=t, stats=False, **kw)
        assert fer[t - 1] == c[0][1] / c[0][0], t
        seen.add(int(c[0][1]))
    assert len(seen) >= 2  # the limit matters at this point


# ------------------------------------------------------------ 6. lifecycle
def _raw_read(dec, point, hist_len, cap):
    hist, und, nf = np.zeros(max(hist_len, 1), np.int64), np.zeros(2, np.int64), np.zeros(2, np.int64)
    rec = np.zeros((max(cap, 1), 2), np.int64)
    rc = _lib.gpu().ldpc_mc_stats_read(dec._h, point, _lib.ptr(hist), hist_len, _lib.ptr(und), _lib.ptr(rec), cap,
                                       _lib.ptr(nf))
    return rc, hist, nf


def test_lifecycle(gpu_available):
    from ldpc_amd.device import Decoder, Graph
    edd = ldpc_amd.load_committed_code(W576)
    dec, gp = Decoder(Graph.cached(edd._h_std), B), Graph.cached(edd.physical_matrix())
    sig = [mc.sigma_for_snr(-2.5)]
    EINVAL = _lib.LDPC_EINVAL

    def refused(fn, *a):
        with pytest.raises(ldpc_amd.LdpcError) as e:
            fn(*a)
        assert e.value.code == EINVAL
        return str(e.value)
    refused(dec.mc_stats_read, 0, T)                          # never enabled
    with pytest.raises(ValueError):
        dec.mc_stats(True, -1)
    assert _lib.gpu().ldpc_mc_stats_enable(dec._h, 1, -1) == EINVAL
    dec.mc_stats(True, B)
    assert "run" in refused(dec.mc_stats_read, 0, T)          # enabled, no run yet
    ctr = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", alpha=ALPHA)
    first = dec.mc_stats_read(0, T)
    ref.assert_identities(first["hist"], ctr[0])
    assert len(first["failed"]) == ctr[0][1] > 8
    refused(dec.mc_stats_read, 1, T)                          # point out of range
    refused(dec.mc_stats_read, -1, T)
    assert "hist_len" in refused(dec.mc_stats_read, 0, T - 1)  # wrong hist_len
    refused(dec.mc_stats_read, 0, T + 1)
    rc, _, _ = _raw_read(dec, 0, T + 1, 8)                    # failed_cap too small
    assert rc == EINVAL and b"failed_cap" in _lib.lib().ldpc_last_error()
    rc, hist, nf = _raw_read(dec, 0, T + 1, B)
    assert rc == 0 and np.array_equal(hist, first["hist"]) and nf.tolist() == [ctr[0][1], 0]
    ref.assert_equal(dec.mc_stats_read(0, T), first, "a second read")  # reading does not reset
    # a second run replaces the first one's statistics
    ctr2 = dec.phys_mc_run(gp, SEED, sig, 64, 5000, 10, cn="nms", schedule="layered", alpha=ALPHA)
    second = dec.mc_stats_read(0, 10)
    ref.assert_identities(second["hist"], ctr2[0])
    assert second["hist"].sum() == 64 and (second["failed"][:, 0] >= 5000).all()
    refused(dec.mc_stats_read, 0, T)                          # the first run's T no longer fits
    # the parity-mode run collects nothing and says so
    pc = dec.mc_run(SEED, sig, 64, 0, 5)
    assert pc[0][0] == 64
    assert "ldpc_mc_run" in refused(dec.mc_stats_read, 0, 5)
    dec.phys_mc_run(gp, SEED, sig, 64, 0, T, cn="nms", alpha=ALPHA)
    assert dec.mc_stats_read(0, T)["hist"].sum() == 64
    dec.mc_stats(False)
    refused(dec.mc_stats_read, 0, T)                          # after a disable
    off = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", alpha=ALPHA)
    assert np.array_equal(off, ctr)
    refused(dec.mc_stats_read, 0, T)


# ------------------------------------------------------------------ 7. CLI
def test_simulate_and_cli(gpu_available, tmp_path, capsys):
    want = [s for s, _ in _want(W576, W576_SNRS, "layered")]
    res, ctr, st = mc.simulate(W576, list(W576_SNRS), B, T, seed=SEED, mode="physical", cn_rule="nms",
                               schedule="layered", alpha=ALPHA, stats=True, max_failed=64)
    assert len(mc.simulate(W576, [0.0], 64, T, seed=SEED, mode="physical", cn_rule="nms")) == 2  # as before
    path = tmp_path / "stats.json"
    mc.main(["--matrix", W576, "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered", "-b", str(B),
             "-i", str(T), "--seed", str(SEED), "--initial-snr", "-2.5", "--end-snr", "0", "--step-snr", "2.5",
             "--stats-json", str(path), "--max-failed", "64"])
    capsys.readouterr()
    doc = json.loads(path.read_text())
    assert doc["seed"] == SEED and [d["snr_db"] for d in doc["points"]] == list(W576_SNRS)
    for p, w in enumerate(want):
        F = int(w["hist"][T])
        by_index = {int(i): int(e) for i, e in w["failed"]}
        for d in (doc["points"][p], {k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in st[p].items()}):
            assert d["hist"] == w["hist"].tolist() and d["frames"] == B
            assert (d["undetected_frames"], d["undetected_bit_errors"]) == \
                (w["undetected_frames"], w["undetected_bit_errors"])
            assert d["fer_by_max_iter"] == mc.fer_by_max_iter(w["hist"]).tolist()
            assert d["fer_by_max_iter"][-1] == res.snr_points[p].fer == ctr[p][1] / B
            assert len(d["failed"]) == min(F, 64) and d["failed_dropped"] == max(F - 64, 0)
            assert all(by_index.get(i) == e for i, e in d["failed"])
            if F <= 64:
                assert d["failed"] == w["failed"].tolist()
    assert want[0]["hist"][T] > 64 and want[1]["hist"][T] == 0  # the list overflows at one point, is empty at the other
