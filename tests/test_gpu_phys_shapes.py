"""Physical mode's kernel variants on irregular graphs (tests/synth_graphs.py:
every register shape, the generic kernels, the HBM path's <8>, <16>, <32>,
long-row and any-degree instantiations, ragged m and n, a column without
edges, layers wider than the block, frames reusing a workgroup's LDS).

The min-sum and fixed-point rules share the kernels' indexing with the
sum-product rule and EQUAL their numpy restatements (minsum_ref, qminsum_ref),
so every indexing branch is checked exactly.  The sum-product rule is then
compared between its own paths bit for bit, and over one and two iterations
with the float64 contract (spa_ref64), within 8 x the error the fp32 libm
restatement (oracle.phys_decode) has on the same case: the GPU replaces libm by
one-instruction exp2 / rcp / log2 of about 1 ulp each and rounds x log2(e) once
more, a small multiple of libm's own error; a wrong term, clamp or sign costs
1e-2 or more against a bound below 8e-4.
Measured on an MI355X (max |GPU - float64| / max |restatement - float64|):
see DESIGN.md "Physical mode: kernel variants on irregular graphs"."""
import numpy as np
import pytest

import ldpc_amd
import spa_ref64
import synth_graphs as sg

GRAPHS = [n for n in sg.NAMES if n != "pairs"]
T = 10


def _graph(name):
    from ldpc_amd.device import Graph
    return Graph.cached(sg.graph(name))


def _committed(name):
    from ldpc_amd.device import Graph
    return Graph.cached(ldpc_amd.load_committed_code(name).physical_matrix())


def _assert_equal(got, want, what, dtype=np.float32):
    for key in ("z", "conv", "status", "iters"):
        assert np.array_equal(got[key], want[key]), \
            f"{what}: {key} differs in {int((np.asarray(got[key]) != want[key]).sum())} places"
    assert got["post"].dtype == dtype and want["post"].dtype == dtype
    bad = got["post"] != want["post"]
    assert not bad.any(), f"{what}: {int(bad.sum())} posteriors differ, first at {np.argwhere(bad)[0].tolist()}"


def _assert_same_bits(a, b, what):
    for key in ("z", "conv", "status", "iters"):
        assert np.array_equal(a[key], b[key]), \
            f"{what}: {key} differs in {int((np.asarray(a[key]) != b[key]).sum())} places"
    bad = a["post"].view(np.uint32) != b["post"].view(np.uint32)
    assert not bad.any(), f"{what}: {int(bad.sum())} posteriors differ, first at {np.argwhere(bad)[0].tolist()}"


def _qkw(cn, param_q):
    """phys_decode's float alpha / beta for the integer parameter."""
    return dict(cn=cn, qbits=sg.QBITS, llr_scale=sg.QSCALE,
                **({"alpha": param_q / 16.0} if cn == "nms" else {"beta": param_q / sg.QSCALE}))


# ------------------------------------------------ the exact rules, every variant
@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_nms_flooding_lds(gpu_available, name):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = sg.ms_ref(name, "nms", "flooding")
    assert sg.both_exits(want)
    g = _graph(name)
    assert phys_kernel_name(g, cn="nms") == sg.KERNELS[name][0]
    got = phys_decode(g, sg.frames(name), T, post=True, cn="nms", alpha=sg.ALPHA)
    _assert_equal(got, want, f"{name} nms lds")


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_oms_flooding_hbm(gpu_available, name):
    """70 noisy frames and the hand-made one: a full 64-frame tile and a ragged
    one.  `ragged` is the regression test of the column without edges, whose
    posterior the HBM variable-node kernel once set to 0 instead of Lambda."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = sg.ms_ref(name, "oms", "flooding")
    assert sg.both_exits(want)
    g = _graph(name)
    assert phys_kernel_name(g, hbm=True, cn="oms") == "phys_cn_tile_kernel"
    hbm = phys_decode(g, sg.frames(name), T, post=True, cn="oms", beta=sg.BETA, hbm=True)
    _assert_equal(hbm, want, f"{name} oms hbm")
    lds = phys_decode(g, sg.frames(name), T, post=True, cn="oms", beta=sg.BETA)
    _assert_same_bits(hbm, lds, f"{name} oms hbm vs lds")
    if name == "ragged":  # L = Lambda on the columns without edges
        lam = -(sg.frames(name).astype(np.float32))
        assert np.array_equal(hbm.post[:, [37, 100]], lam[:, [37, 100]])


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_layered(gpu_available, name):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    cn = sg.LAYERED_RULE[name]
    want = sg.ms_ref(name, cn, "layered")
    assert sg.both_exits(want)
    g = _graph(name)
    assert phys_kernel_name(g, cn=cn, schedule="layered") == "phys_layered_kernel"
    got = phys_decode(g, sg.frames(name), T, post=True, cn=cn, schedule="layered", alpha=sg.ALPHA, beta=sg.BETA)
    _assert_equal(got, want, f"{name} {cn} layered")


Q_ALL = [(name,) + c for name in GRAPHS for c in sg.Q_CASES] + [(sg.Q_OMS_GRAPH, "oms", "flooding", sg.BETA_Q)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,cn,schedule,param_q", Q_ALL)
def test_fixed_point(gpu_available, monkeypatch, name, cn, schedule, param_q):
    """q = 6, scale 4.  Where the register kernel runs, the forced generic one too."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    want = sg.q_ref(name, cn, schedule, param_q)
    assert sg.both_exits(want)
    g = _graph(name)
    kernel = sg.KERNELS[name][1] if schedule == "flooding" else "phys_quant_kernel"
    assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=sg.QBITS) == kernel
    got = phys_decode(g, sg.frames(name), T, post=True, schedule=schedule, **_qkw(cn, param_q))
    _assert_equal(got, want, f"{name} q {cn} {schedule}", np.int16)
    if kernel == "phys_quant_reg_kernel":
        monkeypatch.setenv("LDPC_PHYS_Q_REG", "0")
        assert phys_kernel_name(g, cn=cn, schedule=schedule, qbits=sg.QBITS) == "phys_quant_kernel"
        got = phys_decode(g, sg.frames(name), T, post=True, schedule=schedule, **_qkw(cn, param_q))
        _assert_equal(got, want, f"{name} q {cn} {schedule} generic", np.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("name", GRAPHS)
def test_spa_lds_equals_hbm(gpu_available, name):
    from ldpc_amd.device import phys_decode, phys_kernel_name
    g = _graph(name)
    assert phys_kernel_name(g) == sg.KERNELS[name][0] and phys_kernel_name(g, hbm=True) == "phys_cn_tile_kernel"
    lds = phys_decode(g, sg.frames(name), T, post=True)
    hbm = phys_decode(g, sg.frames(name), T, post=True, hbm=True)
    _assert_same_bits(lds, hbm, f"{name} spa lds vs hbm")
    assert np.isfinite(lds.post).all()


# ------------------------------------- the generic fp32 kernel, forced
def _forced_frames(name):
    if name in sg.NAMES:
        return _graph(name), sg.frames(name)
    import oracle
    from ldpc_amd import montecarlo as mc
    edd = ldpc_amd.load_committed_code(name)
    _, _, llr = oracle.generate_frames(edd._h_std, sg.SEED, 2, mc.sigma_for_snr(-2.5), 0, 70)
    return _committed(name), llr


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "shape2", "deg16", "wimax_576_0.5", "wimax_2304_0.5"])
def test_generic_kernel_equals_register_kernel(gpu_available, monkeypatch, name):
    """LDPC_PHYS_REG=0 (read per launch): phys_kernel on graphs that have a
    register shape -- "identical operations in identical order", all three rules."""
    from ldpc_amd.device import phys_decode, phys_kernel_name
    g, llr = _forced_frames(name)
    rules = (dict(cn="spa"), dict(cn="nms", alpha=sg.ALPHA), dict(cn="oms", beta=sg.BETA))
    assert phys_kernel_name(g) == "phys_reg_kernel"
    reg = [phys_decode(g, llr, T, post=True, **kw) for kw in rules]
    monkeypatch.setenv("LDPC_PHYS_REG", "0")
    assert phys_kernel_name(g) == "phys_kernel" and phys_kernel_name(g, cn="nms") == "phys_kernel"
    for kw, want in zip(rules, reg):
        _assert_same_bits(phys_decode(g, llr, T, post=True, **kw), want, f"{name} {kw['cn']} generic vs register")
    monkeypatch.setenv("LDPC_PHYS_REG", "1")
    assert phys_kernel_name(g) == "phys_reg_kernel"
    if name in sg.NAMES:
        assert sg.both_exits(reg[1]) and np.array_equal(reg[1].post, sg.ms_ref(name, "nms", "flooding")["post"])


# ------------------------------------- many frames per workgroup
# 4133 frames: the LDS kernels launch min(CUs x workgroups per CU, frames)
# workgroups, at most 8 per CU (32 waves / 4), so on a device of <= 256 CUs every
# workgroup decodes two full rounds of frames in the same LDS and 37 a third
# (re-zeroed E, the trailing barrier of frame_finish, s_err reused); the layered
# kernel at one workgroup per CU decodes 16 and more.  The HBM path takes them
# in chunks of 1024: five, the last of 37 frames.
REUSE_FRAMES, REUSE_T = 4133, 8


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ragged", "widecol"])
def test_many_frames_per_workgroup(gpu_available, monkeypatch, name):
    from ldpc_amd.device import phys_decode
    assert REUSE_FRAMES == 2 * 256 * 8 + 37 == 4 * 1024 + 37
    g, llr = _graph(name), sg.frames(name, REUSE_FRAMES, False)
    want = sg.ms_ref(name, "nms", "flooding", REUSE_T, REUSE_FRAMES, False)
    ok = int((want["status"] == 0).sum())
    assert REUSE_FRAMES // 20 < ok < REUSE_FRAMES - REUSE_FRAMES // 20
    got = phys_decode(g, llr, REUSE_T, post=True, cn="nms", alpha=sg.ALPHA)
    _assert_equal(got, want, f"{name} nms lds x{REUSE_FRAMES}")
    monkeypatch.setenv("LDPC_LAYERED_PER_CU", "1")
    got = phys_decode(g, llr, REUSE_T, post=True, cn="nms", schedule="layered", alpha=sg.ALPHA)
    _assert_equal(got, sg.ms_ref(name, "nms", "layered", REUSE_T, REUSE_FRAMES, False), f"{name} layered x{REUSE_FRAMES}")
    got = phys_decode(g, llr, REUSE_T, post=True, cn="oms", beta=sg.BETA, hbm=True)
    _assert_equal(got, sg.ms_ref(name, "oms", "flooding", REUSE_T, REUSE_FRAMES, False), f"{name} oms hbm x{REUSE_FRAMES}")
    _assert_same_bits(phys_decode(g, llr, REUSE_T, post=True), phys_decode(g, llr, REUSE_T, post=True, hbm=True),
                      f"{name} spa lds vs hbm x{REUSE_FRAMES}")


# ------------------------------------- sum-product against float64
def _report(what, got, c, mask=None):
    d = np.abs(got.astype(np.float64) - c["ref"]["post"])
    if mask is not None:
        d = d[mask]
    print(f"{what}: max |GPU - float64| = {d.max():.3g}, max |restatement - float64| = {c['err']:.3g}, "
          f"ratio {d.max() / c['err']:.2f} (bound {sg.SPA_FACTOR:g})")
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("iters", [1, 2])
@pytest.mark.parametrize("name", sg.SPA_GRAPHS)
def test_spa_short_horizon_against_float64(gpu_available, name, iters):
    """8 frames of uniform llr, one iteration ([-6, 6]) and two ([-3, 3]: M = L - E),
    LDS and HBM.  Every posterior of every frame within the bound."""
    from ldpc_amd.device import phys_decode
    c = sg.spa_case(name, iters)
    assert c["err"] < 1e-4
    assert (c["ref"]["margin"] > c["bound"]).all()  # no posterior close enough to 0 for conv to depend on it
    sure = np.abs(c["ref"]["post"]) > c["bound"]
    for hbm in (False, True):
        got = phys_decode(_graph(name), c["llr"], iters, post=True, hbm=hbm)
        what = f"{name} T={iters} {'hbm' if hbm else 'lds'}"
        d = _report(what, got.post, c)
        assert d.max() <= c["bound"], f"{what}: {d.max():.3g} > {c['bound']:.3g} at {np.argwhere(d == d.max())[0].tolist()}"
        assert np.array_equal(got.z[sure], (c["ref"]["post"] >= 0)[sure])
        assert np.array_equal(got.conv, c["oracle"]["conv"]) and np.array_equal(got.iters, c["oracle"]["iters"])
        assert np.array_equal(got.status, c["oracle"]["status"]) and (got.iters == iters).all()


@pytest.mark.gpu
def test_phi_sweep(gpu_available):
    """phi pointwise on `pairs`, one iteration: the even column of row r
    receives sign(x) phi(phi|x|) from its odd neighbour's Lambda = x."""
    from ldpc_amd.device import phys_decode
    c = sg.phi_case()
    x, tight, ref = c["x"], c["tight"], c["ref"]["post"]
    cap = float(spa_ref64.phi(0.0)) + 1e-3
    for hbm in (False, True):
        got = phys_decode(_graph("pairs"), c["llr"], 1, post=True, hbm=hbm)
        what = f"phi sweep {'hbm' if hbm else 'lds'}"
        post = got.post.astype(np.float64)
        d = _report(what, got.post, c, tight)
        assert d.max() <= c["bound"], f"{what}: {d.max():.3g} > {c['bound']:.3g}"
        sure = np.abs(ref) > c["bound"]
        assert np.array_equal(got.z[sure & tight], (ref >= 0)[sure & tight])
        assert np.array_equal(got.conv, c["oracle"]["conv"]) and np.array_equal(got.iters, c["oracle"]["iters"])
        for i, own in enumerate(sg.PHI_OWN):
            E = post[i, 0::2] - own  # exact: own and the fp32 posterior are float64 values
            # sign (that of x; M < 0 is false for +0.0 and -0.0: positive) and range, for every |x|
            Es = np.where(x < 0, -E, E)
            assert (Es >= 0).all() and (Es <= cap).all(), what
            if own == 0.5:  # phi(phi(1e-7)) ~ 1e-7 is two ulp of 0.5: the sign of the smallest message shows
                assert (Es[np.abs(x) <= 1e-7] > 0).all() and (E[x == 0] > 0).all(), what
            # from 8 on fp32 phi is quantised by design: |E| only must not decrease as |x| grows
            for neg in (False, True):
                rows = np.nonzero((np.abs(x) >= 8.0) & ((x < 0) == neg))[0]
                rows = rows[np.argsort(np.abs(x[rows]))]
                print(f"{what} own {own} {'-' if neg else '+'}|x| >= 8: |E| =", np.abs(E[rows]).tolist())
                assert len(rows) == len(sg.PHI_BIG) and (np.diff(np.abs(E[rows])) >= 0).all(), (what, own, neg)
            # from 30 on e^x +- 1 is e^x in fp32, and a quotient within an ulp of 1 makes phi|x| at most
            # 2^-23 ln 2, so S - phi(own) is at most one ulp of phi(0.5), 2^-23: the message is phi at its
            # lower clamp, or phi(2^-23) = 16.64 -- a lower clamp anywhere else shows here
            assert (np.abs(E[np.abs(x) >= 30.0]) >= float(spa_ref64.phi(2.0 ** -23)) - 1e-3).all(), what
            # the odd columns received +phi(phi(own)): never below their Lambda, never more than the cap above
            Eo = post[i, 1::2] - x.astype(np.float32).astype(np.float64)
            assert (Eo >= 0).all() and (Eo <= cap).all(), what
