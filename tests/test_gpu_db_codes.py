"""The parity decoder on the reference database's other code shapes.

Every other GPU parity test takes its graph from one of the five shipped
codes.  The ten of tests/db_codes.py sit on the limits the kernel choice
branches on (tile64_lds_bytes, sub_lds_bytes_q<4>, t8_variant, cn_sub_shape,
use_cn_row / use_cn_row16, edge_slots / small_batch_edge, small_batch_cols,
lpt_weak_id, the packed encoder table); tests/test_db_codes_host.py pins the
CPU oracle to the reference's own decode of each of them, and here the oracle
is the reference.

ROUTES, below, is written out by hand from those predicates (the LDS budgets
in bytes are in DESIGN.md "Parity decoder on the database's other shapes"),
not by asking the library; test_route_table holds the library to it.
  T64   tile_kernel codes (k <= 320, rows <= 192, 512 k + ... <= 160 KiB of
        LDS): edge (up to 4 frames by default), split, tile.  No second
        layout: tile8 is never chosen where tile_kernel applies.
  SUB   rows 193..640 and 128 k + ... <= 160 KiB: tile_sub_kernel by default;
        created with LDPC_TILE8=1 the graph is tile8_kernel's (K = 5, L_A in
        LDS), and its pair form fits too -- as wimax_2304_0.5.
  wimax_2304_0.66B  rows of 644 > 640: neither sub16 nor tile8's K = 5 / pair
        forms; tile8 K = 8 (rows <= 1024, 64 k + ... fits) by default, no
        tile-resident decoder in the 64-frame layout -- as the r3/4 codes.
  wimax_2304_0.83   rows of 1030: C = ceil(1030 / 16) = 65 > 64 excludes tile8
        K = 8 too, cn_sub_shape is 0 and the edge path (<= 1024) is off: only
        the split CN (cn_kernel) with vn_cols_kernel or vn_kernel.
"""
import numpy as np
import pytest

import oracle
from conftest import assert_llr_close, max_rel
from db_codes import CODES, SET_OF, SHAPES, db_hstd, load_db_golden
from test_gpu_decoders import _ALL, _graph, _run_route
from test_gpu_parity import _random_llr

pytestmark = pytest.mark.gpu

SEED = 20260213

T64 = ("CCSDS_ldpc_n32_k16", "Tanner_155_64", "WRAN_N480_K240_R05")
SUB = ("WRAN_N384_K320_R083", "wigig_R05_N672_K336", "ieee_802_11ad_n672_r081", "wimax_1152_0.83", "wimax_1440_0.5")

# code -> ({graph layout: ldpc_tile_kernel_name}, ldpc_cn_kernel_name, [(route, layout)])
# layouts as test_gpu_decoders._graph: None = default, 8 = LDPC_TILE8=1, "8p" = + LDPC_T8_PAIR=1, 64 = LDPC_TILE8=0
ROUTES = {}
for _c in T64:
    ROUTES[_c] = ({None: "tile_kernel", 8: "tile_kernel", 64: "tile_kernel"}, "cn_row_kernel",
                  [("edge", None), ("split", None), ("tile", None)])
for _c in SUB:
    ROUTES[_c] = ({None: "tile_sub_kernel", 64: "tile_sub_kernel", 8: "tile8_kernel", "8p": "tile8_kernel:pair"},
                  "cn_kernel",
                  [("edge", None), ("cols", None), ("split", None), ("tile", None),
                   ("tile", 8), ("split", 8), ("tile", "8p")])
ROUTES["wimax_2304_0.66B"] = ({None: "tile8_kernel", 8: "tile8_kernel", "8p": "tile8_kernel", 64: ""}, "cn_kernel",
                              [("edge", None), ("cols", None), ("split", None), ("tile", None),
                               ("split", 64), ("cols", 64)])
ROUTES["wimax_2304_0.83"] = ({None: "", 8: "", 64: ""}, "cn_kernel", [("cols", None), ("split", None)])
assert sorted(ROUTES) == sorted(CODES)

# Routes that cannot serve a shape -> the kinds the call runs instead:
# forced to the edge path, wimax_2304_0.83 (rows of 1030 > 1024) falls to the
# split CN + column-parallel VN; asked for the tile-resident decoder it has
# none and runs the split CN + vn_kernel.
INSTEAD = {("wimax_2304_0.83", "edge"): ("cn", "vn_cols"), ("wimax_2304_0.83", "tile"): ("cn", "vn")}

# Kinds of the unforced Decoder.decode of 1 and of 5 frames (main.py's call
# pattern): the edge path up to 4 frames where tile_kernel applies and up to
# 32 elsewhere; wimax_2304_0.83 has no edge path.
EDGE, TILE, COLS = ("cn_edge", "vn_edge"), ("tile",), ("cn", "vn_cols")
UNFORCED = {c: (EDGE, TILE) if c in T64 else (COLS, COLS) if c == "wimax_2304_0.83" else (EDGE, EDGE) for c in CODES}

# 70 random-codeword frames at T = 6: the SNR at which the ORACLE converges on
# some and not on others (chosen on the CPU; asserted on the oracle's output)
SNR70 = {"CCSDS_ldpc_n32_k16": -2.0, "Tanner_155_64": 1.0, "WRAN_N480_K240_R05": 2.0, "WRAN_N384_K320_R083": 1.5,
         "wigig_R05_N672_K336": 2.0, "ieee_802_11ad_n672_r081": 2.0, "wimax_1152_0.83": 2.0, "wimax_1440_0.5": 2.0,
         "wimax_2304_0.66B": 2.0, "wimax_2304_0.83": 2.5}
B70, T70 = 70, 6


def _id(route, layout):
    return f"{route}{'' if layout is None else layout}"


def _names(g):
    from ldpc_amd import _lib
    return (_lib.lib().ldpc_tile_kernel_name(g.handle).decode(), _lib.lib().ldpc_cn_kernel_name(g.handle).decode())


@pytest.mark.parametrize("code", CODES)
def test_route_table(gpu_available, monkeypatch, code):
    """The hand-written table against what the library reports for each graph layout."""
    tiles, cn, _ = ROUTES[code]
    for layout, want in tiles.items():
        g = _graph(code, layout, monkeypatch)
        got_tile, got_cn = _names(g)
        print(f"{code} layout={layout}: tile={got_tile!r} cn={got_cn!r} rows<={g.max_row_deg} cols<={g.max_col_deg}")
        assert (got_tile, got_cn) == (want, cn), (code, layout)
        assert (g.k, g.m, g.max_row_deg, g.max_col_deg) == (SHAPES[code][0], SHAPES[code][1], SHAPES[code][3],
                                                            SHAPES[code][4])


_SLACK = {}


def _slack(code, llr, T, nllr, key):
    if key not in _SLACK:
        _SLACK[key] = oracle.conditioning_slack(db_hstd(code), llr, T, nllr=nllr)
    return _SLACK[key]


_GOLDEN = [(c, r, lay) for c in CODES for (r, lay) in ROUTES[c][2]] + [(c, r, None) for (c, r) in INSTEAD]


@pytest.mark.parametrize("code,route,layout", _GOLDEN, ids=[f"{c}-{_id(r, l)}" for c, r, l in _GOLDEN])
def test_golden_through_every_decoder(gpu_available, monkeypatch, code, route, layout):
    """The reference's own decode of each code through every route that serves
    it (test_gpu_decoders.test_golden_through_every_decoder's assertions)."""
    g = load_db_golden(SET_OF[code])
    nl, T = bool(g["nllr_on"]), int(g["T"])
    r = _run_route(code, layout, route, g["ch"], T, monkeypatch, tile_name=ROUTES[code][0][layout],
                   instead=INSTEAD.get((code, route)), nllr=nl, post=True, hist=nl, msgs=True)
    np.testing.assert_array_equal(r.z, g["z"], err_msg="hard decisions")
    np.testing.assert_array_equal(r.conv, g["conv"], err_msg="convergence_iteration")
    np.testing.assert_array_equal(r.status == 0, g["ok"], err_msg="Result")
    np.testing.assert_array_equal(r.iters, np.where(g["conv"] >= 0, g["conv"] + 1, T))
    if nl:
        np.testing.assert_array_equal(r.nllr, g["nllr"], err_msg="normalized LLR")
    es = int(g["e_stride"])
    print(f"{code} {_id(route, layout)}: max rel |L - reference| = {max_rel(r.post, g['L']):.3e}")
    try:  # plain 1e-5 first; the measured one-ulp slack only where that fails (saturated frames)
        assert_llr_close(r.post, g["L"], "posterior L")
        assert_llr_close(r.msgs[:, ::es], g["E"], "messages E")
    except AssertionError:
        sl_L, sl_E = _slack(code, g["ch"], T, nl, ("golden", code))
        assert_llr_close(r.post, g["L"], "posterior L", slack=sl_L)
        assert_llr_close(r.msgs[:, ::es], g["E"], "messages E", slack=sl_E[:, ::es])


def _against_oracle(r, o, code, llr, T, key, what):
    for k in ("z", "conv", "status", "iters", "nllr"):
        np.testing.assert_array_equal(r[k], o[k], err_msg=f"{what}: {k}")
    try:
        assert_llr_close(r.post, o["post"], f"{what}: posterior L")
        if r.msgs is not None:
            assert_llr_close(r.msgs, o["msgs"], f"{what}: messages E")
    except AssertionError:
        sl_L, sl_E = _slack(code, llr, T, True, key)
        assert_llr_close(r.post, o["post"], f"{what}: posterior L", slack=sl_L)
        if r.msgs is not None:
            assert_llr_close(r.msgs, o["msgs"], f"{what}: messages E", slack=sl_E)


@pytest.mark.parametrize("code", CODES)
def test_70_frames_every_route(gpu_available, monkeypatch, code):
    """One full 64-frame tile and a ragged one of random codewords, T = 6,
    through every serving route: each equal to the oracle (z, conv, status,
    iterations, nllr exact; L and E within 1e-5) and all routes bit-identical
    to one another in L and E."""
    H = db_hstd(code)
    llr = _random_llr(H, B70, SNR70[code], seed=7000 + CODES.index(code))
    o = oracle.spa_decode(H, llr, T70, nllr=True, want_E=True)
    ok = int((o["status"] == 0).sum())
    assert 3 <= ok <= B70 - 3, (code, ok)  # both exits, by the oracle (synth_graphs.both_exits)
    first = None
    for route, layout in ROUTES[code][2]:
        r = _run_route(code, layout, route, llr, T70, monkeypatch, tile_name=ROUTES[code][0][layout],
                       nllr=True, post=True, msgs=True)
        print(f"{code} {_id(route, layout)}: {ok}/{B70} converge; max rel |L - oracle| = "
              f"{max_rel(r.post, o['post']):.3e}, |E - oracle| = {max_rel(r.msgs, o['msgs']):.3e}")
        _against_oracle(r, o, code, llr, T70, ("70", code), _id(route, layout))
        if first is None:
            first = (route, layout, r)
            continue
        for k in ("post", "msgs", "z", "conv", "status", "iters", "nllr"):
            np.testing.assert_array_equal(r[k], first[2][k],
                                          err_msg=f"{k}: {_id(route, layout)} vs {_id(*first[:2])}")


@pytest.mark.parametrize("code", CODES)
def test_unforced_decode_of_one_and_five_frames(gpu_available, monkeypatch, code):
    """main.py's call pattern: Decoder.decode of 1 frame and of 5, nothing forced."""
    from ldpc_amd.device import Decoder
    H = db_hstd(code)
    llr = _random_llr(H, B70, SNR70[code], seed=7000 + CODES.index(code))
    T = T70
    dec = Decoder(_graph(code, None, monkeypatch), 64)
    for B, must in zip((1, 5), UNFORCED[code]):
        # 5 frames that hold both exits where the first five do not
        o_all = oracle.spa_decode(H, llr, T, nllr=True)
        pick = np.arange(B) if B == 1 else np.concatenate([np.nonzero(o_all["status"] == 0)[0][:2],
                                                            np.nonzero(o_all["status"] != 0)[0][:3]])
        x = llr[pick]
        o = oracle.spa_decode(H, x, T, nllr=True, want_E=True)
        dec.profile(True)
        r = dec.decode(x, T, nllr=True, post=True, msgs=True)
        p = dec.profile_read()
        dec.profile(False)
        print(f"{code} B={B}: ran {[k for k in _ALL if p[k][1] > 0]}")
        for kind in _ALL:
            assert (p[kind][1] > 0) == (kind in must), (code, B, kind, p)
        _against_oracle(r, o, code, x, T, ("unforced", code, B), f"B={B}")
    dec.close()


@pytest.mark.parametrize("code", ["CCSDS_ldpc_n32_k16", "Tanner_155_64", "ieee_802_11ad_n672_r081",
                                  "wimax_2304_0.83"])
def test_frame_source(gpu_available, monkeypatch, code):
    """The packed encoder table and the u-bit words: k = 16 (half a word),
    64 (exactly two), 546 (17 words + 2 bits), 1920 (60 words, A rows of up to
    1029 bits) -- u exact, LLRs to the ulp of log/cos/sin."""
    from ldpc_amd.device import Decoder
    H = db_hstd(code)
    dec = Decoder(_graph(code, None, monkeypatch), B70)
    sigma = oracle.sigma_for_snr(2.0)
    u, llr = dec.generate(SEED, 3, sigma, 1000, B70)
    uo, co, lo = oracle.generate_frames(H, SEED, 3, sigma, 1000, B70)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
    assert uo.any() and not uo.all()
    assert not ((H @ co.T.astype(np.int64)) % 2).any()
    dec.close()


# code, SNR points, the tile-resident streaming kernel's graph reports
_MC = [
    ("WRAN_N480_K240_R05", (1.5, 3.0), "tile_kernel"),        # tile_stream_kernel, lpt_weak_id = 0
    ("WRAN_N384_K320_R083", (1.0, 2.0), "tile_sub_kernel"),   # the smallest code on the sub-tile stream
    ("wigig_R05_N672_K336", (1.5, 3.0), "tile_sub_kernel"),   # sub-tile stream, rows of 193
    ("wimax_2304_0.66B", (2.0, 2.5), "tile8_kernel"),         # tile8_stream_kernel, K = 8
    ("wimax_2304_0.83", (2.0, 2.5), ""),                      # no tile kernel: the split streaming loop
]
MC_CAP, MC_FRAMES, MC_T = 128, 200, 8


@pytest.mark.parametrize("code,snrs,tile", _MC, ids=[m[0] for m in _MC])
def test_mc_three_schedules_equal_oracle(gpu_available, monkeypatch, code, snrs, tile):
    """ldpc_mc_run of 200 frames through 128 slots (slots refill), T = 8: the
    streaming schedule, the static one and the split streaming loop give the
    same counters, which are main.py's applied to the oracle's decode of the
    frames generate() returns."""
    from ldpc_amd.device import Decoder
    H = db_hstd(code)
    k = H.shape[1] - H.shape[0]
    g = _graph(code, None, monkeypatch)
    assert _names(g)[0] == tile
    monkeypatch.setenv("LDPC_HANDOFF", "0")
    dec = Decoder(g, MC_CAP)
    sig = [oracle.sigma_for_snr(s) for s in snrs]
    dec.profile(True)
    a = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True)
    p = dec.profile_read()
    dec.profile(False)
    print(f"{code}: streaming ran {[(kd, p[kd][1]) for kd in _ALL if p[kd][1] > 0]}")
    if tile:
        assert p["tile"][1] == len(snrs) and p["cn"][1] == 0, p  # one tile launch per point
    else:  # cn_kernel + the column-parallel tail VN (2 tiles <= kTailTiles)
        assert p["tile"][1] == 0 and p["cn"][1] > 0 and p["vn_cols"][1] == p["cn"][1] and p["vn"][1] == 0, p
    b = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True, static=True)
    c = dec.mc_run(SEED, sig, MC_FRAMES, 3, MC_T, nllr=True, split=True)
    np.testing.assert_array_equal(a, b, err_msg="streaming vs static")
    np.testing.assert_array_equal(a, c, err_msg="streaming vs split streaming")
    assert (a[:, 0] == MC_FRAMES).all()
    dec.close()
    gen = Decoder(g, MC_FRAMES)
    for i, s in enumerate(sig):
        u, llr = gen.generate(SEED, i, s, 3, MC_FRAMES)
        o = oracle.spa_decode(H, llr, MC_T, nllr=True)
        want = oracle.main_counters(u, o["z"], o["status"], o["conv"],
                                    nllr_cnt=np.rint(o["nllr"] * k).astype(np.int64), iters=o["iters"])
        np.testing.assert_array_equal(a[i], want, err_msg=f"point {i}")
    gen.close()


def test_frame_order_without_the_weak_identity_key(gpu_available, monkeypatch):
    """WRAN_N480_K240: 140 of 240 rows have odd degree, so lpt_weak_id = 0 and
    the supply order is the stable descending ranking by syndrome weight alone
    -- a permutation of the frame range, equal to the host's ranking."""
    from ldpc_amd.device import Decoder
    code = "WRAN_N480_K240_R05"
    H = db_hstd(code).tocsr()
    m, n = H.shape
    assert 2 * int((np.diff(H.indptr) & 1).sum()) > m
    sig = oracle.sigma_for_snr(2.0)
    frame0, count = 123457, 500
    dec = Decoder(_graph(code, None, monkeypatch), 64)
    order = dec.frame_order(SEED, 2, sig, frame0, count)
    dec.close()
    np.testing.assert_array_equal(np.sort(order), np.arange(count))
    _, _, llr = oracle.generate_frames(H, SEED, 2, sig, frame0, count)
    hard = (llr > 0.0).astype(np.int64)
    w = np.asarray(((H @ hard.T) % 2).sum(axis=0)).ravel().astype(np.int64)
    np.testing.assert_array_equal(order, np.argsort(-w, kind="stable"))
    assert len(np.unique(w)) < count  # ties exist: the order within them is the frame index's
