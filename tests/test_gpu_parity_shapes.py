"""The parity decoder on graphs that sit exactly on, and one edge over, each
limit of its kernel choice (tests/parity_graphs.py): max_row_deg 192 / 640 /
960 / 1024, k = 2048 and max_col_deg = 1024; an empty A column; a row with its
identity entry only.  70 frames at T = 4 through every route the predicates
admit, each against oracle.spa_decode (z, conv, status, iterations, nllr
exact; L and E within 1e-5) and all routes bit-identical to one another; the
kernel names and the profile's kinds against the table below.

The table is derived by hand from csrc's predicates (classes as in
tests/test_gpu_db_codes.py; LDS totals in DESIGN.md):
  r192k288  rows <= 192 and 512*288 + ... = 158,496 B <= 160 KiB: tile_kernel.
  r193k288  one edge more: tile64_lds_bytes = 0; sub16 (128 k + ... fits).
  r192      k = 320: rows would allow tile_kernel but its S alone is 163,840 B
            (the k <= 320 clause never decides: LDS stops at k = 302) -> sub16;
            rows <= 192: cn_row_kernel.       r193: cn_kernel.
  r640      sub16, tile8 K = 5 and its pair form all hold 640 = 16*4*10 =
            16*8*5.                           r641: only tile8 K = 8.
  r960 / r961 / r1024   tile8 K = 8 (rows <= 16*8*8); cn_sub shape 30 up to
            960, cn_kernel above (both report "cn_kernel": use_cn_row is false).
  r1025     ceil(1025/16) = 65 > 64: no tile-resident decoder; no edge path.
  k2048     tile8 K = 8 (64 k + ... = 147,120 B); edge and column-parallel
            paths hold k = 2048 = 64 words.
  k2049     65 words: neither small-batch path (cols_ok is false), so every
            unforced call runs tile8_kernel, which has no such limit.
  c1024     k = 40: tile_kernel; the edge path holds columns of 1024 = 64*16.
  c1025     the edge path is off; the unforced call runs tile_kernel.
"""
import numpy as np
import pytest

import oracle
import parity_graphs as pg
from conftest import assert_llr_close, max_rel
from test_gpu_db_codes import TILE, _id, _names
from test_gpu_decoders import _ALL, _graph, _run_route

pytestmark = pytest.mark.gpu

SEED = 20260213
R_T64 = [("edge", None), ("split", None), ("tile", None)]
R_SUB = [("edge", None), ("cols", None), ("split", None), ("tile", None), ("tile", 8), ("split", 8), ("tile", "8p")]
R_T8 = [("edge", None), ("cols", None), ("split", None), ("tile", None), ("split", 64), ("cols", 64)]
N_T64 = {None: "tile_kernel", 8: "tile_kernel", 64: "tile_kernel"}
N_SUB = {None: "tile_sub_kernel", 64: "tile_sub_kernel", 8: "tile8_kernel", "8p": "tile8_kernel:pair"}
N_T8 = {None: "tile8_kernel", 8: "tile8_kernel", "8p": "tile8_kernel", 64: ""}

# graph -> ({layout: ldpc_tile_kernel_name}, ldpc_cn_kernel_name, [(route, layout)])
ROUTES = {
    "r192k288": (N_T64, "cn_row_kernel", R_T64),
    "r193k288": (N_SUB, "cn_kernel", R_SUB),
    "r192": (N_SUB, "cn_row_kernel", R_SUB),
    "r193": (N_SUB, "cn_kernel", R_SUB),
    "r640": (N_SUB, "cn_kernel", R_SUB),
    "r641": (N_T8, "cn_kernel", R_T8),
    "r960": (N_T8, "cn_kernel", R_T8),
    "r961": (N_T8, "cn_kernel", R_T8),
    "r1024": (N_T8, "cn_kernel", R_T8),
    "r1025": ({None: "", 8: "", 64: ""}, "cn_kernel", [("cols", None), ("split", None)]),
    "k2048": (N_T8, "cn_row_kernel", R_T8),
    "k2049": (N_T8, "cn_row_kernel", [("split", None), ("tile", None), ("split", 64)]),
    "c1024": (N_T64, "cn_row_kernel", R_T64),
    "c1025": (N_T64, "cn_row_kernel", [("split", None), ("tile", None)]),
    "emptycol": (N_T64, "cn_row_kernel", R_T64),
    "idrow": (N_T64, "cn_row_kernel", R_T64),
}
assert sorted(ROUTES) == sorted(pg.NAMES)

# forced routes that cannot serve a graph: (graph, route, layout, the kinds the call runs instead)
INSTEAD = [
    ("r1025", "edge", None, ("cn", "vn_cols")),   # rows of 1025: the split CN + column-parallel VN
    ("r1025", "tile", None, ("cn", "vn")),        # no tile-resident decoder
    ("k2049", "edge", None, TILE),                # 65 words of (z^1)_A: tile8_kernel takes the call
    ("k2049", "cols", None, TILE),
    ("k2049", "cols", 64, ("cn", "vn")),          # ... and in the 64-frame layout the split CN + vn_kernel
    ("c1025", "edge", None, TILE),                # a column of 1025: tile_kernel
]


@pytest.mark.parametrize("name", pg.NAMES)
def test_route_table(gpu_available, monkeypatch, name):
    tiles, cn, _ = ROUTES[name]
    k, m, _, rows, cols = pg.shape(name)
    for layout, want in tiles.items():
        g = _graph(name, layout, monkeypatch)
        got = _names(g)
        print(f"{name} layout={layout}: tile={got[0]!r} cn={got[1]!r} rows<={g.max_row_deg} cols<={g.max_col_deg}")
        assert got == (want, cn), (name, layout)
        assert (g.k, g.m, g.max_row_deg, g.max_col_deg) == (k, m, rows, cols)


def _against_oracle(r, o, what):
    for key in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(r[key], o[key], err_msg=f"{what}: {key}")
    assert_llr_close(r.post, o["post"], f"{what}: posterior L")
    if r.msgs is not None:
        assert_llr_close(r.msgs, o["msgs"], f"{what}: messages E")


@pytest.mark.parametrize("name", pg.NAMES)
def test_70_frames_every_route(gpu_available, monkeypatch, name):
    llr, o = pg.frames(name), pg.reference(name)
    assert pg.both_exits(o), name
    first = None
    forced = [(r, lay, None) for r, lay in ROUTES[name][2]]
    forced += [(r, lay, must) for n, r, lay, must in INSTEAD if n == name]
    for route, layout, instead in forced:
        r = _run_route(name, layout, route, llr, pg.T, monkeypatch, tile_name=ROUTES[name][0][layout],
                       instead=instead, nllr=True, post=True, msgs=True)
        tag = _id(route, layout) + ("" if instead is None else f" -> {'+'.join(instead)}")
        print(f"{name} {tag}: {int((o['status'] == 0).sum())}/{pg.FRAMES} converge; max rel |L - oracle| = "
              f"{max_rel(r.post, o['post']):.3e}, |E - oracle| = {max_rel(r.msgs, o['msgs']):.3e}")
        _against_oracle(r, o, f"{name} {tag}")
        if first is None:
            first = (tag, r)
            continue
        for key in ("post", "msgs", "z", "conv", "status", "iters", "nllr"):
            np.testing.assert_array_equal(r[key], first[1][key], err_msg=f"{name} {key}: {tag} vs {first[0]}")


# The two graphs no small-batch route holds.  Whatever the C ABI does for
# them must be a correct decode on a route without that limit (or an LDPC_E*
# return); as the code stands it is the former, on these kinds:
#   graph -> (unforced decode, decode(split=True), streaming mc_run, split streaming mc_run)
ROUTELESS = {
    "k2049": (TILE, ("cn", "vn"), TILE, ("cn", "vn")),          # tail_ok is false: vn_kernel, never vn_cols_kernel
    "c1025": (TILE, ("cn", "vn"), TILE, ("cn", "vn_cols")),     # the column-parallel tail has no column limit
}
MC_CAP, MC_FRAMES, MC_T = 128, 200, 4


def _kinds(p):
    return tuple(k for k in _ALL if p[k][1] > 0)


@pytest.mark.parametrize("name", list(ROUTELESS))
def test_routeless_graphs_decode_correctly(gpu_available, monkeypatch, name):
    from ldpc_amd.device import Decoder
    unforced, split, stream, split_stream = ROUTELESS[name]
    H, llr, o = pg.graph(name), pg.frames(name), pg.reference(name)
    g = _graph(name, None, monkeypatch)
    dec = Decoder(g, MC_CAP)
    dec.profile(True)
    # main.py's one-frame call, a few frames (where the edge path would run) and the 70
    for pick in (np.arange(1), np.array([0, 1, 40, 41, 69]), np.arange(pg.FRAMES)):
        for sp, must in ((False, unforced), (True, split)):
            r = dec.decode(llr[pick], pg.T, nllr=True, post=True, msgs=True, split=sp)
            p = dec.profile_read()
            print(f"{name} B={len(pick)} split={sp}: ran {_kinds(p)}")
            assert _kinds(p) == must, (name, len(pick), sp, p)
            _against_oracle(r, {k: v[pick] for k, v in o.items()}, f"{name} B={len(pick)} split={sp}")
    # Monte-Carlo: 200 frames through 128 slots, the three schedules and the oracle
    monkeypatch.setenv("LDPC_HANDOFF", "0")
    sig = [oracle.sigma_for_snr(s) for s in pg.SNRS[name]]
    a = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True)
    p = dec.profile_read()
    print(f"{name}: streaming ran {_kinds(p)}")
    assert _kinds(p) == stream and p["tile"][1] == len(sig), p
    b = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True, static=True)
    dec.profile_read()
    c = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True, split=True)
    p = dec.profile_read()
    print(f"{name}: split streaming ran {_kinds(p)}")
    assert _kinds(p) == split_stream, p
    dec.profile(False)
    dec.close()
    np.testing.assert_array_equal(a, b, err_msg="streaming vs static")
    np.testing.assert_array_equal(a, c, err_msg="streaming vs split streaming")
    gen = Decoder(g, MC_FRAMES)
    k = H.shape[1] - H.shape[0]
    for i, s in enumerate(sig):
        u, fl = gen.generate(SEED, i, s, 3, MC_FRAMES)
        uo, _, lo = oracle.generate_frames(H, SEED, i, s, 3, MC_FRAMES)
        np.testing.assert_array_equal(u, uo)
        np.testing.assert_allclose(fl, lo, rtol=1e-12, atol=1e-12)
        od = oracle.spa_decode(H, fl, MC_T, nllr=True)
        want = oracle.main_counters(u, od["z"], od["status"], od["conv"],
                                    nllr_cnt=np.rint(od["nllr"] * k).astype(np.int64), iters=od["iters"])
        np.testing.assert_array_equal(a[i], want, err_msg=f"point {i}")
    gen.close()
    order = Decoder(g, 64)
    np.testing.assert_array_equal(np.sort(order.frame_order(SEED, 0, sig[0], 3, 300)), np.arange(300))
    order.close()
