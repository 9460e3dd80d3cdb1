"""The synthetic graphs of tests/synth_graphs.py hold the structures they are
named for, their frames exercise both exits of every restatement used on them,
and the float64 sum-product reference (tests/spa_ref64.py) agrees with the fp32
libm restatement within the margin the GPU tests build their bound on.  No GPU.

The kernel each graph must reach is worked out here from the matrix with the
dispatch rules restated (csrc/phys_kernels.hip:reg_shape, csrc/phys_quant.hip:
phys_quant_reg_shape, csrc/phys_tile.hip:launch_cn_tile_rule / launch_phys_tile_vn)
and compared with synth_graphs' table; tests/test_gpu_phys_shapes.py asserts
the same names against the library."""
import numpy as np
import pytest

import ldpc_amd
import minsum_ref
import spa_ref64
import synth_graphs as sg
from ldpc_amd.device import validate_csr

# phys_kernels.hip:kRegShapes -- {rows per thread, row degree, columns per
# thread, column degree} of phys_reg_kernel at 512 threads.  A graph takes the
# shape that covers it (rpt >= ceil(m / 512), cpt >= ceil(n / 512), rdeg >= max
# row degree, cdeg >= max column degree) with the fewest index registers
# rpt * rdeg + cpt * cdeg (the first on a tie); none, or nnz or n >= 65536: the
# generic phys_kernel.
REG_SHAPES = ((1, 8, 1, 8), (1, 8, 2, 8), (2, 8, 3, 8), (2, 16, 5, 8), (3, 8, 5, 8))
# phys_quant.hip:kQRegShapes -- {rows per thread, dwords per row, columns per
# thread, column degree} of phys_quant_reg_kernel (flooding, 512 threads, the
# frame's state within 65536 bytes): rpt * 512 >= m, cpt * 512 >= n, 4 rw >= max
# row degree, cdeg >= max column degree; cost rpt * rw * 2 + cpt * cdeg.
QREG_SHAPES = ((1, 2, 2, 6), (3, 2, 5, 6))


def reg_shape(H):
    rd, cd = sg.degrees(H)
    m, n = H.shape
    if H.nnz >= 65536 or n >= 65536:
        return None
    rpt, cpt = -(-m // 512), -(-n // 512)
    fits = [s for s in REG_SHAPES if s[0] >= rpt and s[2] >= cpt and s[1] >= rd.max() and s[3] >= cd.max()]
    return min(fits, key=lambda s: s[0] * s[1] + s[2] * s[3]) if fits else None


def qreg_shape(H):
    rd, cd = sg.degrees(H)
    m, n = H.shape
    epad = int(((rd + 3) // 4 * 4).sum())
    if epad + ((2 * n + 2 + 3) & ~3) + ((n + 3) & ~3) > 65536:
        return None
    fits = [s for s in QREG_SHAPES if s[0] * 512 >= m and s[2] * 512 >= n and 4 * s[1] >= rd.max() and s[3] >= cd.max()]
    return min(fits, key=lambda s: s[0] * s[1] * 2 + s[2] * s[3]) if fits else None


def _hist(d):
    return dict(zip(*(a.tolist() for a in np.unique(d, return_counts=True))))


# name -> (m, n, the row degrees (exactly these occur), column degrees that must occur,
#          max column degree, register shape, fixed-point register shape, HBM check kernel's kDeg, HBM VN kCD)
WANT = {
    "ragged": (37, 101, {2, 3, 5, 7, 8}, {0, 1, 8}, 8, (1, 8, 1, 8), None, 8, 8),
    "shape2": (700, 1400, {5, 6, 7, 8}, {6}, 6, (2, 8, 3, 8), (3, 2, 5, 6), 8, 8),
    "deg16": (520, 2100, {9, 11, 15, 16}, set(), 8, (2, 16, 5, 8), None, 16, 8),
    "widecol": (61, 121, {3, 4, 5, 6}, {9, 12}, 12, None, None, 8, 0),
    "longrow": (200, 1203, {17, 24, 32, 33, 40}, set(), 8, None, None, 32, 8),
    "large": (1300, 2602, {6, 7}, set(), 8, None, None, 8, 8),
    "widelayer": (1200, 2400, {5}, set(), 8, (3, 8, 5, 8), (3, 2, 5, 6), 8, 8),
    "pairs": (256, 512, {2}, {1}, 1, (1, 8, 1, 8), (1, 2, 2, 6), 8, 8),
}


@pytest.mark.parametrize("name", sg.NAMES)
def test_structure(name):
    H = sg.graph(name)
    m, n, rows, cols, max_col, reg, qreg, kdeg, kcd = WANT[name]
    rd, cd = sg.degrees(H)
    assert H.shape == (m, n) and m <= n and H.has_sorted_indices
    for r in range(m):
        assert (np.diff(H.indices[H.indptr[r]:H.indptr[r + 1]]) > 0).all()
    assert set(_hist(rd)) == rows and rd.min() >= 2, _hist(rd)
    assert cols <= set(_hist(cd)) and cd.max() <= max_col, _hist(cd)
    assert reg_shape(H) == reg and qreg_shape(H) == qreg
    assert sg.KERNELS[name] == ("phys_reg_kernel" if reg else "phys_kernel",
                                "phys_quant_reg_kernel" if qreg else "phys_quant_kernel")
    # HBM path: phys_cn_tile_kernel<8 | 16 | 32> by the longest row (rows past 32 take its two-sweep
    # branch), phys_vn_tile_kernel<8> up to column degree 8, else <0>
    assert (8 if rd.max() <= 8 else 16 if rd.max() <= 16 else 32) == kdeg
    assert (8 if cd.max() <= 8 else 0) == kcd
    validate_csr(m, n, H.indptr, H.indices)  # what ldpc_graph_create checks


def test_named_edges_are_present():
    rd, cd = sg.degrees(sg.graph("ragged"))
    # rows of exactly RDEG = 8 and of 2 and 3 (a 16-bit pair with a missing high half); a column of
    # exactly CDEG = 8; columns without edges, one of them the last; m % 16 and n % 32 ragged
    assert {2, 3, 8} <= set(rd.tolist()) and (cd == 8).sum() == 1 and cd[100] == 0 and cd[37] == 0
    assert 37 % 16 and 101 % 32 and 101 % 8
    rd, cd = sg.degrees(sg.graph("deg16"))
    assert rd.max() == 16 and {9, 11} <= set(rd.tolist())  # exactly RDEG = 16; dword tails of 1 and 3
    assert 520 % 16 and 2100 % 32
    rd, cd = sg.degrees(sg.graph("widecol"))
    assert cd[120] == 12 and cd[8] == 9  # the wide column is the last, in the ragged column block
    rd, cd = sg.degrees(sg.graph("longrow"))
    assert (rd > 32).any() and (rd == 32).any() and ((rd > 16) & (rd < 32)).any() and 1203 % 8
    # `large`: more columns than 5 x 512 (no register shape, n past the fixed-point one's 2560), and
    # the generic kernels' 256 threads take several rows each
    assert -(-2602 // 512) == 6 and 1300 > 4 * 256
    assert sg.degrees(sg.graph("shape2"))[1][1399] == 6  # the fixed-point register kernel's column bound


@pytest.mark.parametrize("name", ["widelayer", "large", "ragged"])
def test_layers(name):
    H = sg.graph(name)
    lp, lr = minsum_ref.first_fit_layers(H)
    bp, br = ldpc_amd.build_layers(H)
    np.testing.assert_array_equal(lp, bp)
    np.testing.assert_array_equal(lr, br)
    if name != "ragged":  # a layer wider than the 256-thread block: the layer loop's second trip
        assert np.diff(lp).max() > 256
    if name == "widelayer":
        assert np.diff(lp).tolist() == [300, 300, 300, 300]


@pytest.mark.parametrize("name", [n for n in sg.NAMES if n != "pairs"])
def test_frames_take_both_exits(name):
    llr = sg.frames(name)
    assert llr.shape == (sg.FRAMES + 1, sg.graph(name).shape[1])
    for label, r in sg.exact_cases(name):
        assert sg.both_exits(r), (name, label, int((r["status"][:sg.FRAMES] == 0).sum()))


def test_hand_frame():
    H = sg.graph("ragged")
    base = sg.noisy_frames(101, 0.8, 1, 1)[0]
    f = sg.hand_frame(H, base)
    changed = np.nonzero((f != base) | (np.signbit(f) != np.signbit(base)))[0]
    want = [v for grp in sg.HAND_GROUPS for v in grp]
    for v in want:
        assert ((f == v) & (np.signbit(f) == np.signbit(v))).any(), v
    assert np.float32(1e-40) != 0 and np.float32(1e-40) < np.finfo(np.float32).tiny  # denormal in fp32
    # each group sits inside one row, and the tie is that row's smallest pair
    for grp in sg.HAND_GROUPS:
        rows = [r for r in range(H.shape[0])
                if all(any(f[c] == v and np.signbit(f[c]) == np.signbit(v)
                           for c in H.indices[H.indptr[r]:H.indptr[r + 1]]) for v in grp)]
        assert rows, grp
    tie = sg.HAND_GROUPS[sg.HAND_TIE]
    r = next(r for r in range(H.shape[0]) if {tie[0], tie[1]} <= set(f[H.indices[H.indptr[r]:H.indptr[r + 1]]]))
    a = np.sort(np.abs(f[H.indices[H.indptr[r]:H.indptr[r + 1]]]))
    assert a[0] == a[1] == abs(tie[0]) and (len(a) == 2 or a[2] > a[1])
    assert len(changed) <= sum(len(g) for g in sg.HAND_GROUPS) + 8


# ---- the float64 sum-product reference
def test_phi64():
    x = np.array([1e-9, 1e-7, 1e-3, 0.03125, 0.5, 4.0, 12.0, 30.0, 50.0])
    p = spa_ref64.phi(x)
    xc = np.clip(x, spa_ref64.PHI_MIN, 30.0)
    np.testing.assert_allclose(p[:7], -np.log(np.tanh(xc[:7] / 2)), rtol=1e-9)  # the definition, where tanh resolves it
    np.testing.assert_allclose(p[-1], 2 * np.exp(-30.0), rtol=1e-12)  # phi(x) -> 2 e^-x
    assert p[0] == p[1] and p[-1] == p[-2] and 16.8 < p[0] < 16.82
    mid = x[2:7]
    np.testing.assert_allclose(spa_ref64.phi(spa_ref64.phi(mid)), mid, rtol=1e-9)  # self-inverse


def test_ref64_by_hand():
    """One row [a, b, c]: E_a = sign(b c) phi(phi|b| + phi|c|), the tanh rule."""
    H = np.array([[1, 1, 1, 0], [0, 0, 1, 1]])
    lam = np.array([[0.75, -1.875, 2.5, -0.25]])  # exact in fp32
    r = spa_ref64.decode(H, -lam, 1)
    t = np.tanh(lam[0] / 2)
    want = lam[0] + np.array([2 * np.arctanh(t[1] * t[2]), 2 * np.arctanh(t[0] * t[2]),
                              2 * np.arctanh(t[0] * t[1]) + 2 * np.arctanh(t[3]), 2 * np.arctanh(t[2])])
    np.testing.assert_allclose(r["post"][0], want, rtol=1e-12)
    assert (want < 0).tolist() == [True, True, False, False] and r["conv"][0] == 0  # both rows' parity even
    assert spa_ref64.decode(H, -np.array([[0.75, 1.875, 2.5, -2.75]]), 1)["conv"][0] == -1  # b = [0, 0, 0, 1]
    two = spa_ref64.decode(H, -lam, 2)
    assert two["post"].shape == (1, 4) and not np.allclose(two["post"], r["post"])


@pytest.mark.parametrize("T", [1, 2])
@pytest.mark.parametrize("name", sg.SPA_GRAPHS)
def test_restatement_error_against_float64(name, T):
    """The GPU tests' bound is 8 x this error; it must stay below 1e-4 (bound
    below 8e-4) for a wrong term, clamp or sign (>= 1e-2) to be told apart."""
    c = sg.spa_case(name, T)
    print(f"{name} T={T}: max |fp32 libm restatement - float64| = {c['err']:.3g}")
    assert 0.0 < c["err"] < 1e-4
    # every frame runs the full T in both (no early exit changes what is compared)
    assert np.isin(c["ref"]["conv"], (-1, T - 1)).all() and (c["oracle"]["iters"] == T).all()
    # no posterior of any iteration is close enough to 0 for a hard decision, and with it conv, to
    # depend on the last bits: the GPU's conv and iters must equal the restatement's on every frame
    assert (c["ref"]["margin"] > c["bound"]).all()
    np.testing.assert_array_equal(c["oracle"]["conv"], c["ref"]["conv"])


def test_phi_sweep_restatement_error():
    c = sg.phi_case()
    print(f"phi sweep: max |fp32 libm restatement - float64| = {c['err']:.3g} where the bound applies, "
          f"{c['err_loose']:.3g} elsewhere")
    assert 0.0 < c["err"] < 1e-4 and c["err_loose"] < 0.5
    x, ref = c["x"], c["ref"]["post"]
    # both posteriors of a row are own + x up to the clamps: the same sign, far from 0, so every frame
    # satisfies every check after its one iteration whatever the last bits are
    assert (c["ref"]["margin"] > 20 * c["bound"]).all()
    assert (c["ref"]["conv"] == 0).all() and (c["oracle"]["conv"] == 0).all() and (c["oracle"]["iters"] == 1).all()
    assert (x == 0).sum() == 2 and np.signbit(x[x == 0]).tolist() == [False, True]
    assert (np.abs(x) == np.float32(0.03125)).sum() == 2
    # the even column of row r receives sign(x) phi(phi|x|): |x| itself inside the clamps
    for i, own in enumerate(sg.PHI_OWN):
        E = ref[i, 0::2] - own
        inside = (np.abs(x) >= 1e-3) & (np.abs(x) < 8)
        np.testing.assert_allclose(E[inside], x[inside], rtol=1e-6)
        assert (E[x == 0] > 0).all()  # +0.0 and -0.0: M < 0 is false for both
