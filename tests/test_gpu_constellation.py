"""The physical-mode frame source under a constellation table
(ldpc_constellation_set: 2^bps complex points, demapped over all of them) on
the GPU.

1. generate() against the numpy restatement (tests/constellation_ref.py) for
   8PSK, 16APSK, random 32- and 64-point tables and a 2-point table, both
   models, both demappers, on wimax_576_0.5, an IRA graph and an [A | I] graph
   of 14 symbols;
2. a table that spells out QPSK / 16-QAM / 64-QAM gives the built-in
   modulation's frames;
3. the built-in labellings are the right model: sign errors per bit position
   against the quadrature of nearest-point decisions;
4. under a pattern, an interleaver, block fading and HARQ plans;
5. the three output forms carry the same frames: the Monte-Carlo counters of
   every decoder path equal the restatements' on the frames generate() returns;
6. the refusals leave the decoder usable;
7. with no table set, nothing moved.
"""
import ctypes
import functools

import numpy as np
import pytest
from scipy import sparse, stats

import bitflip_ref
import channel_ref
import constellation_ref
import ldpc_amd
import mc_stats_ref
import minsum_ref
import oracle
import qminsum_ref
import ratematch_ref
from conftest import hstd_for
from ldpc_amd import _lib, interleave
from ldpc_amd import montecarlo as mc
from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
from ldpc_amd.constellation import Constellation
from ldpc_amd.harq import HarqPlan
from ldpc_amd.ratematch import RateMatch

pytestmark = pytest.mark.gpu

SEED = 20260213
ALPHA, BETA = 0.75, 0.5
W576 = "wimax_576_0.5"


def _random_table(bps, seed):
    rng = np.random.default_rng(seed)
    return Constellation.from_points(list(rng.normal(size=1 << bps) + 1j * rng.normal(size=1 << bps)),
                                     name=f"rand{1 << bps}")


TABLES = {
    "8psk": Constellation.psk8(),
    "16apsk": Constellation.apsk16(),
    "rand32": _random_table(5, 32),
    "rand64": _random_table(6, 64),
    "two": Constellation.from_points([1.0 + 0.5j, -0.7 - 0.2j], name="two"),  # not antipodal, not real
}
# the generator test's noise per bps: LLRs of a few units, every decision in play
GEN_SIGMA = {1: 0.8, 2: 0.6, 3: 0.4, 4: 0.3, 5: 0.2, 6: 0.15}
SPECS = [(model, demap) for model in ("awgn", "rayleigh") for demap in ("exact", "maxlog")]


def _pts(table):
    return np.array(table.points)


def tiny_graph(m, n, seed):
    """[A | I_m] with k = n - m information columns, three A entries a row."""
    k = n - m
    rng = np.random.default_rng(seed)
    rows, cols = [], []
    for r in range(m):
        for c in sorted(rng.choice(k, 3, replace=False)):
            rows.append(r)
            cols.append(int(c))
        rows.append(r)
        cols.append(k + r)
    return sparse.csr_matrix((np.ones(len(rows), np.int8), (rows, cols)), shape=(m, n))


@functools.lru_cache(maxsize=None)
def _graph_h(name):
    """(H the frame source encodes with, ira)."""
    if name == "tiny70":
        return tiny_graph(20, 70, 70), False
    if name == "ira1440":
        from ldpc_amd import ira
        return sparse.csr_matrix(ira.small_ira_matrix()), True
    return hstd_for(name), False


_DECODERS = {}


def _decoder(name, frames):
    """One decoder per graph and size for the whole module (closed by _close_decoders)."""
    from ldpc_amd.device import Decoder, Graph
    if (name, frames) not in _DECODERS:
        _DECODERS[name, frames] = Decoder(Graph.cached(_graph_h(name)[0]), frames)
    return _DECODERS[name, frames]


@pytest.fixture(scope="module", autouse=True)
def _close_decoders():
    yield
    for dec in _DECODERS.values():
        dec.close()
    _DECODERS.clear()


class _under:
    """The decoder under a channel, a table and the other settings; all cleared on exit."""

    def __init__(self, dec, model, demap, table, rm=None, il=None, block=1, plan=None, modulation="bpsk"):
        self.dec, self.args = dec, (ChannelSpec(model, modulation, demap), table, rm, il, block, plan)

    def __enter__(self):
        spec, table, rm, il, block, plan = self.args
        self.dec.set_channel(spec)
        self.dec.set_constellation(table)
        self.dec.set_rate_match(rm)
        self.dec.set_interleaver(il)
        self.dec.set_fading_block(block)
        self.dec.set_harq(plan)
        return self.dec

    def __exit__(self, *exc):
        self.dec.set_harq(None)
        self.dec.set_fading_block(1)
        self.dec.set_interleaver(None)
        self.dec.set_rate_match(None)
        self.dec.set_constellation(None)
        self.dec.set_channel(None)


@functools.lru_cache(maxsize=None)
def _bits(name, snr_point, frame0, count):
    """(u, codeword) of the frames, from the committed CPU frame source."""
    H, ira = _graph_h(name)
    u, c, _ = oracle.generate_frames(H, SEED, snr_point, 1.0, frame0, count, ira=ira)
    u.setflags(write=False)
    c.setflags(write=False)
    return u, c


@functools.lru_cache(maxsize=None)
def _ref(name, table, model, demap, snr_point, sigma, frame0, count):
    llr, bound = constellation_ref.frames(_pts(TABLES[table]), model, demap, _bits(name, snr_point, frame0, count)[1],
                                          None, SEED, snr_point, sigma, frame0)
    llr.setflags(write=False)
    bound.setflags(write=False)
    return llr, bound


def _assert_close(llr, want, bound, what, factor=1.0):
    assert np.isfinite(llr).all(), what
    ratio = float((np.abs(llr - want) / (factor * bound)).max())
    print(f"{what}: max |delta| / bound = {ratio:.3g}")
    assert ratio <= 1.0, f"{what}: |delta| is {ratio:.3g} x the bound"


# ------------------------------------------------------------ 1. generator
GEN_CASES = [(W576, "8psk"), ("ira1440", "8psk"), (W576, "16apsk"), ("ira1440", "rand32"), ("tiny70", "rand32"),
             (W576, "two"), (W576, "rand64")]


@pytest.mark.parametrize("model,demap", SPECS, ids=[f"{m}-{d}" for m, d in SPECS])
@pytest.mark.parametrize("name,table", GEN_CASES, ids=[f"{n}-{t}" for n, t in GEN_CASES])
def test_generator_matches_restatement(gpu_available, name, table, model, demap):
    """70 frames (a full tile and a ragged one) from frame 1000 of SNR point 3:
    u and the codeword identical, |llr - restatement| <= 1e-12 max(1, M) +
    1e-12 |llr| with M the frame's largest per-axis metric, every LLR finite,
    and at sigma = 1e-6 (class minima some 1e11 apart) the signs are the
    codeword."""
    count, frame0, p = 70, 1000, 3
    tab = TABLES[table]
    sigma = GEN_SIGMA[tab.bps]
    dec = _decoder(name, 128)
    with _under(dec, model, demap, tab):
        got = dec.constellation
        assert got.points == tab.points and got.bps == tab.bps and got.name == tab.name
        assert dec.channel == ChannelSpec(model, "bpsk", demap)  # ldpc_channel_get keeps reporting what was set
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
        _, quiet = dec.generate(SEED, p, 1e-6, frame0, count)
    uo, co = _bits(name, p, frame0, count)
    np.testing.assert_array_equal(u, uo)
    assert np.isfinite(quiet).all()
    # a fade h < 1e-4, where the noise could still decide, has probability 1e-8 a symbol
    np.testing.assert_array_equal(quiet > 0, co == 1)
    want, bound = _ref(name, table, model, demap, p, sigma, frame0, count)
    _assert_close(llr, want, bound, f"{name} {table} {model} {demap}")


# ------------------------------------------------- 2. table against built-in
@pytest.mark.parametrize("model,demap", SPECS, ids=[f"{m}-{d}" for m, d in SPECS])
@pytest.mark.parametrize("mod,bps", [("qpsk", 2), ("qam16", 4), ("qam64", 6)])
def test_spelled_out_qam_gives_the_built_in_frames(gpu_available, mod, bps, model, demap):
    """The same frames by two routes (per axis, and over all points), each
    within the bound of the restatement: within twice the bound of each other,
    and the same hard decisions wherever |llr| exceeds it."""
    count, frame0, p = 70, 1000, 3
    sigma = GEN_SIGMA[bps]
    pts, _ = channel_ref.constellation(bps)
    tab = Constellation.from_points(list(pts), name=f"{mod}-table", normalize=False)
    dec = _decoder(W576, 128)
    with _under(dec, model, demap, None, modulation=mod):
        u0, built_in = dec.generate(SEED, p, sigma, frame0, count)
    with _under(dec, model, demap, tab):  # the channel's modulation stays BPSK: the table replaces it
        u1, table = dec.generate(SEED, p, sigma, frame0, count)
    np.testing.assert_array_equal(u0, u1)
    _, M = channel_ref.frames_llr(ChannelSpec(model, mod, demap), _bits(W576, p, frame0, count)[1], SEED, p, sigma,
                                  frame0)
    bound = 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(built_in)
    _assert_close(table, built_in, bound, f"{mod} {model} {demap}", factor=2.0)
    sure = np.abs(built_in) > 2.0 * bound
    np.testing.assert_array_equal((table > 0)[sure], (built_in > 0)[sure])
    assert sure.mean() > 0.99


# ------------------------------------------- 3. the labellings are the right model
@pytest.mark.parametrize("table,sigma", [("8psk", 0.30), ("16apsk", 0.25)])
def test_sign_errors_match_expected_ber(gpu_available, table, sigma):
    """96 frames, AWGN, max-log (its sign is the nearest-point decision): the
    errors of every bit position lie in the central 99.9 % binomial interval of
    constellation_ref.expected_ber -- and so do the restatement's own."""
    count, p = 96, 1
    tab = TABLES[table]
    rate = constellation_ref.expected_ber(_pts(tab), sigma)
    dec = _decoder(W576, 128)
    with _under(dec, "awgn", "maxlog", tab):
        _, llr = dec.generate(SEED, p, sigma, 0, count)
    c = _bits(W576, p, 0, count)[1]
    ref = _ref(W576, table, "awgn", "maxlog", p, sigma, 0, count)[0]
    pos = np.arange(c.shape[1]) % tab.bps
    N = (c.shape[1] // tab.bps) * count
    for t in range(tab.bps):
        g = int(((llr > 0) != (c == 1))[:, pos == t].sum())
        r = int(((ref > 0) != (c == 1))[:, pos == t].sum())
        lo, hi = stats.binom.ppf(0.0005, N, rate[t]), stats.binom.ppf(0.9995, N, rate[t])
        print(f"{table} a{t}: device {g}, restatement {r} of {N}; expected {rate[t] * N:.1f}, band [{lo:.0f}, {hi:.0f}]")
        assert lo <= r <= hi, f"restatement, bit a{t}"
        assert lo <= g <= hi, f"device, bit a{t}"


# ------------------------------------------------------------ 4. composition
RM_8PSK = RateMatch(tuple(range(288, 576, 12)), (0, 1, 2))   # E = 576 - 24 - 3 = 549 = 3 * 183
IL_576 = interleave.random(576, 7)
COMPOSE = {
    # name: (table, model, demap, pattern, interleaver, block_len, plan)
    "puncture-shorten-8psk": ("8psk", "rayleigh", "exact", RM_8PSK, None, 1, None),
    "random7-16apsk": ("16apsk", "awgn", "exact", None, IL_576, 1, None),
    "block7-random7-8psk": ("8psk", "rayleigh", "maxlog", None, IL_576, 7, None),
    "chase2-16apsk": ("16apsk", "awgn", "maxlog", None, None, 1, HarqPlan.chase(576, 2)),
    "ir3x240-16apsk": ("16apsk", "rayleigh", "exact", None, None, 5, HarqPlan.ir(576, 3, 240)),
}


def _tx_lists(case):
    _, _, _, rm, il, _, plan = COMPOSE[case]
    if plan is not None:
        return [list(t) for t in plan.tx]
    tx = np.array(rm.transmitted(576) if rm is not None else range(576), np.int64)
    return [tx[list(il.perm)] if il is not None else tx]


@functools.lru_cache(maxsize=None)
def _compose_bits(case, p, frame0, count):
    rm = COMPOSE[case][3]
    if rm is None:
        return _bits(W576, p, frame0, count)
    return ratematch_ref.bits(hstd_for(W576), False, rm, SEED, p, frame0, count)


@pytest.mark.parametrize("case", list(COMPOSE))
def test_composition_matches_restatement(gpu_available, case):
    """The table under a pattern, an interleaver, a coherence length and HARQ
    plans: the restatement is the list of columns in air order per
    transmission, its bound the per-transmission bound summed over the
    transmissions that carry a column."""
    table, model, demap, rm, il, block, plan = COMPOSE[case]
    count, frame0, p = 70, 1000, 3
    tab = TABLES[table]
    sigma = GEN_SIGMA[tab.bps]
    dec = _decoder(W576, 128)
    with _under(dec, model, demap, tab, rm, il, block, plan):
        u, llr = dec.generate(SEED, p, sigma, frame0, count)
    uo, co = _compose_bits(case, p, frame0, count)
    np.testing.assert_array_equal(u, uo)
    shortened = rm.shortened if rm is not None else ()
    want, bound = constellation_ref.frames(_pts(tab), model, demap, co, _tx_lists(case), SEED, p, sigma, frame0,
                                           fade_block=block, shortened=shortened)
    sent = sorted(set().union(*[set(map(int, t)) for t in _tx_lists(case)]))
    _assert_close(llr[:, sent], want[:, sent], bound[:, sent], case)
    rest = sorted(set(range(576)) - set(sent))
    np.testing.assert_array_equal(llr[:, rest], want[:, rest])  # +0.0 not sent, -LDPC_RM_KNOWN_LLR shortened
    if rm is not None:
        assert (llr[:, list(rm.punctured)] == 0).all() and (llr[:, list(rm.shortened)] == -1.0e4).all()


@pytest.mark.parametrize("case", ["block7-random7-8psk", "ir3x240-16apsk"])
def test_composition_forms_carry_the_same_frames(gpu_available, case):
    """fp32 rows (the LDS decoder) and fp32 tiles (the HBM decoder) under an
    interleaver with block fading and under a HARQ plan: the counters are the
    restatement's on the fp64 frames generate() returns."""
    from ldpc_amd.device import Graph
    table, model, demap, rm, il, block, plan = COMPOSE[case]
    tab = TABLES[table]
    B, T = 96, 10
    sig = [sigma_for_ebn0(e, 0.5, tab.bps, table=True) for e in (9.0, 14.0)]
    Hp = _w576()[1]
    gp = Graph.cached(Hp)
    dec = _decoder(W576, 128)
    with _under(dec, model, demap, tab, rm, il, block, plan):
        frames = [dec.generate(SEED, p, s, 0, B) for p, s in enumerate(sig)]
        rows = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", schedule="layered", alpha=ALPHA)
        tiles = dec.phys_mc_run(gp, SEED, sig, B, 0, T, cn="nms", schedule="flooding", alpha=ALPHA, hbm=True)
    for p, (u, llr) in enumerate(frames):
        o = minsum_ref.decode(Hp, llr, T, "nms", "layered", ALPHA, BETA)
        np.testing.assert_array_equal(rows[p][[0, 1, 2, 3, 4, 6]], _counters(u, o), err_msg=f"{case} rows point {p}")
        o = minsum_ref.decode(Hp, llr, T, "nms", "flooding", ALPHA, BETA)
        np.testing.assert_array_equal(tiles[p][[0, 1, 2, 3, 4, 6]], _counters(u, o), err_msg=f"{case} tiles point {p}")


# ------------------------------- 5. all three output forms carry the same frames
# (model, table, demap): Eb/N0 (dB) of a point inside the waterfall, then an error-free one, found on the CPU
# with the restatement (200 frames, T = 20, NMS; failures of flooding / layered / 6-bit layered at the first
# point: 3 / 2 / 16 and 19 / 10 / 71)
MC_CASES = {("awgn", "8psk", "exact"): (4.0, 8.0),
            ("rayleigh", "16apsk", "maxlog"): (7.0, 14.0)}
MC_B, MC_T = 200, 20
MC_Q_SCALE = 0.5  # as tests/test_gpu_channel.py: a demapper's LLRs reach tens to hundreds here


def _mc_id(case):
    return "-".join(case)


@functools.lru_cache(maxsize=None)
def _w576():
    edd = ldpc_amd.load_committed_code(W576)
    return edd, edd.physical_matrix()


def _mc_sigmas(case):
    edd, _ = _w576()
    return [sigma_for_ebn0(e, edd._k / edd._n, TABLES[case[1]].bps, table=True) for e in MC_CASES[case]]


@functools.lru_cache(maxsize=None)
def _mc_frames(case):
    """The frames generate() returns at the case's two points (read-only), checked against the restatement."""
    model, table, demap = case
    dec = _decoder(W576, 256)
    with _under(dec, model, demap, TABLES[table]):
        out = [dec.generate(SEED, p, s, 0, MC_B) for p, s in enumerate(_mc_sigmas(case))]
    for p, (u, llr) in enumerate(out):
        want, bound = _ref(W576, table, model, demap, p, _mc_sigmas(case)[p], 0, MC_B)
        np.testing.assert_array_equal(u, _bits(W576, p, 0, MC_B)[0])
        assert (np.abs(llr - want) <= bound).all(), (case, p)
        u.setflags(write=False)
        llr.setflags(write=False)
    return out


def _counters(u, o):
    return oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])[[0, 1, 2, 3, 4, 6]]


@functools.lru_cache(maxsize=None)
def _mc_want(case, schedule, qbits=None):
    """Per point: (the restatement's result, its counters) on _mc_frames."""
    Hp = _w576()[1]
    out = []
    for u, llr in _mc_frames(case):
        if qbits is None:
            o = minsum_ref.decode(Hp, llr, MC_T, "nms", schedule, ALPHA, BETA)
        else:
            o = qminsum_ref.decode(Hp, llr, MC_T, "nms", schedule, qbits, MC_Q_SCALE, 12)
        out.append((o, _counters(u, o)))
    # the first point is inside the waterfall, the second is error-free
    assert 0 < out[0][1][1] < MC_B, (case, schedule, qbits, out[0][1])
    assert out[1][1][1] == 0, (case, schedule, qbits, out[1][1])
    return out


MC_PATHS = [("flooding", {}), ("layered", {}), ("flooding", {"hbm": True}), ("layered", {"tile": True})]


@pytest.mark.parametrize("case", list(MC_CASES), ids=_mc_id)
@pytest.mark.parametrize("schedule,flags", MC_PATHS, ids=["flooding-lds", "layered-lds", "flooding-hbm", "layered-tile"])
def test_monte_carlo_counters_equal_restatement(gpu_available, case, schedule, flags):
    from ldpc_amd.device import Graph
    model, table, demap = case
    dec = _decoder(W576, 256)
    gp = Graph.cached(_w576()[1])
    want = _mc_want(case, schedule)
    with _under(dec, model, demap, TABLES[table]):
        got = dec.phys_mc_run(gp, SEED, _mc_sigmas(case), MC_B, 0, MC_T, cn="nms", schedule=schedule, alpha=ALPHA,
                              **flags)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"{_mc_id(case)} {schedule} {flags} point {p}")


def test_fixed_point_and_bit_flipping_counters_equal_restatement(gpu_available):
    """The 6-bit layered decoder on its tiles, and the bit-flipping decoder
    (weight 0.5: 200 and 131 of the 200 frames fail in the restatement)."""
    from ldpc_amd.device import Graph
    case = ("awgn", "8psk", "exact")
    dec = _decoder(W576, 256)
    Hp = _w576()[1]
    gp = Graph.cached(Hp)
    want = _mc_want(case, "layered", 6)
    with _under(dec, case[0], case[2], TABLES[case[1]]):
        got = dec.phys_mc_run(gp, SEED, _mc_sigmas(case), MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA,
                              qbits=6, llr_scale=MC_Q_SCALE, qtile=True)
        bf = dec.bitflip_mc_run(gp, SEED, _mc_sigmas(case), MC_B, 0, MC_T, weight=0.5)
    for p, (_, w) in enumerate(want):
        np.testing.assert_array_equal(got[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"q6 tile point {p}")
    for p, (u, llr) in enumerate(_mc_frames(case)):
        o = bitflip_ref.decode(Hp, llr, MC_T, 0.5, 0.0)
        np.testing.assert_array_equal(bf[p][[0, 1, 2, 3, 4, 6]], _counters(u, o), err_msg=f"bit flipping point {p}")
    assert 0 < bf[1][1] < MC_B


def test_simulate_statistics_and_failed_frames(gpu_available):
    """mc.simulate on the Eb/N0 axis (the table's bps) reproduces the counters
    and the statistics; every failed-frame record regenerates, on that decoder,
    to the frame the restatement also fails."""
    from ldpc_amd.device import Graph
    case = ("rayleigh", "16apsk", "maxlog")
    model, table, demap = case
    want = _mc_want(case, "layered")
    res, ctr, st = mc.simulate(W576, list(MC_CASES[case]), MC_B, MC_T, seed=SEED, mode="physical", cn_rule="nms",
                               schedule="layered", alpha=ALPHA, channel=ChannelSpec(model, "bpsk", demap),
                               snr_axis="ebn0", stats=True, max_failed=MC_B, constellation=TABLES[table])
    for p, ((o, w), (u, _)) in enumerate(zip(want, _mc_frames(case))):
        np.testing.assert_array_equal(ctr[p][[0, 1, 2, 3, 4, 6]], w, err_msg=f"simulate point {p}")
        ws = mc_stats_ref.stats(u, o, MC_T)
        np.testing.assert_array_equal(st[p]["hist"], ws["hist"])
        np.testing.assert_array_equal(st[p]["failed"], ws["failed"])
        assert (st[p]["undetected_frames"], st[p]["undetected_bit_errors"]) == \
            (ws["undetected_frames"], ws["undetected_bit_errors"])
        mc_stats_ref.assert_identities(st[p]["hist"], ctr[p])
    dec = _decoder(W576, 256)
    gp, Hp = Graph.cached(_w576()[1]), _w576()[1]
    sig = _mc_sigmas(case)
    with _under(dec, model, demap, TABLES[table]):
        dec.mc_stats(True, 8)
        try:
            got = dec.phys_mc_run(gp, SEED, sig, MC_B, 0, MC_T, cn="nms", schedule="layered", alpha=ALPHA)
            np.testing.assert_array_equal(got[0][[0, 1, 2, 3, 4, 6]], want[0][1])
            rec = dec.mc_stats_read(0, MC_T)
            assert len(rec["failed"]) == min(8, int(want[0][1][1])) and len(rec["failed"]) > 0
            for index, errs in rec["failed"]:
                u, llr = dec.generate(SEED, 0, sig[0], int(index), 1)
                np.testing.assert_array_equal(llr[0], _mc_frames(case)[0][1][int(index)])
                o = minsum_ref.decode(Hp, llr, MC_T, "nms", "layered", ALPHA, BETA)
                assert o["status"][0] != 0, f"frame {index} does not fail in the restatement"
                assert int(((o["z"][0, :u.shape[1]] ^ 1) != u[0]).sum()) == int(errs)
        finally:
            dec.mc_stats(False)


# ------------------------------------------------------------ 6. refusals
def _einval(call, *needles):
    with pytest.raises(_lib.LdpcError) as e:
        call()
    assert e.value.code == _lib.LDPC_EINVAL, e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def test_setter_refusals_keep_the_earlier_table(gpu_available):
    """ldpc_constellation_set / _get through ctypes on a live decoder: what is
    refused leaves the table that was set in force."""
    L = _lib.lib()
    dec = _decoder(W576, 128)
    p8 = TABLES["8psk"]
    dec.set_constellation(p8)
    try:
        def raw(bps, vals):
            arr = None if vals is None else (ctypes.c_double * len(vals))(*vals)
            return L.ldpc_constellation_set(dec._h, bps, arr)
        unit = [1.0, 0.0, 0.0, 1.0, -1.0, 0.0, 0.0, -1.0]
        for what, bps, vals, msg in (("bps < 0", -1, unit, b"outside"), ("bps = 7", 7, unit, b"outside"),
                                     ("NULL points", 2, None, b"NULL points"),
                                     ("NaN", 2, unit[:5] + [float("nan")] + unit[6:], b"not finite"),
                                     ("inf", 2, [float("inf")] + unit[1:], b"not finite"),
                                     ("energy", 2, [x * (1 + 1e-8) for x in unit], b"mean energy"),
                                     ("duplicate", 2, unit[:6] + unit[:2], b"equal")):
            assert raw(bps, vals) == _lib.LDPC_EINVAL, what
            assert msg in L.ldpc_last_error(), (what, L.ldpc_last_error())
            assert dec.constellation.points == p8.points, what
        bps = ctypes.c_int32(0)
        out = (ctypes.c_double * 16)()
        assert L.ldpc_constellation_get(dec._h, ctypes.byref(bps), None, 0) == 0 and bps.value == 3
        assert L.ldpc_constellation_get(dec._h, ctypes.byref(bps), out, 15) == _lib.LDPC_EINVAL
        assert b"capacity 15" in L.ldpc_last_error()
        assert L.ldpc_constellation_get(dec._h, None, out, 16) == _lib.LDPC_EINVAL
        assert L.ldpc_constellation_get(dec._h, ctypes.byref(bps), out, 16) == 0 and list(out) == p8.flat()
        assert raw(2, [x * (1 + 1e-11) for x in unit]) == 0 and dec.constellation.bps == 2  # within 1e-9
        with pytest.raises(ValueError):
            dec.set_constellation("8psk")
        assert dec.constellation.bps == 2
    finally:
        dec.set_constellation(None)
    assert dec.constellation is None
    assert L.ldpc_constellation_get(dec._h, ctypes.byref(bps), out, 0) == 0 and bps.value == 0


def test_refusals_leave_the_decoder_usable(gpu_available):
    from ldpc_amd.device import Decoder, Graph
    p8, a16 = TABLES["8psk"], TABLES["16apsk"]
    clear = "ldpc_constellation_set(d, 0, NULL)"
    dec = _decoder(W576, 128)
    gp = Graph.cached(_w576()[1])
    # a table under the reference channel
    dec.set_constellation(p8)
    try:
        _einval(lambda: dec.generate(SEED, 0, 0.5, 0, 8), "constellation table", "reference channel", clear)
        _einval(lambda: dec.phys_mc_run(gp, SEED, [0.5], 8, 0, 5), "constellation table", "reference channel", clear)
        _einval(lambda: dec.bitflip_mc_run(gp, SEED, [0.5], 8, 0, 5), "constellation table", clear)
        # parity mode, while a table is set (whatever the channel)
        for spec in (None, ChannelSpec("awgn")):
            dec.set_channel(spec)
            _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5), "parity mode", "constellation table", clear)
            _einval(lambda: dec.mc_run(SEED, [0.8], 64, 0, 5, static=True), "parity mode", clear)
            _einval(lambda: dec.frame_order(SEED, 0, 0.8, 0, 64), "parity mode", clear)
        # the test erasures
        _einval(lambda: dec.generate(SEED, 0, 0.3, 0, 8, test_zero=True), "LDPC_F_TEST_ZERO", "constellation table", clear)
        # E and E_r against the table's bps
        dec.set_rate_match(RateMatch((575,), ()))
        _einval(lambda: dec.generate(SEED, 0, 0.3, 0, 8), "E = 575", "bps = 3", clear)
        dec.set_rate_match(None)
        dec.set_harq(HarqPlan.ir(576, 2, 100))
        _einval(lambda: dec.generate(SEED, 0, 0.3, 0, 8), "E_r = 100", "bps = 3", clear)
        dec.set_harq(None)
        u, llr = dec.generate(SEED, 3, GEN_SIGMA[3], 1000, 70)  # still usable under the table ...
        np.testing.assert_array_equal(u, _bits(W576, 3, 1000, 70)[0])
        want, bound = _ref(W576, "8psk", "awgn", "exact", 3, GEN_SIGMA[3], 1000, 70)
        assert (np.abs(llr - want) <= bound).all()
        # ... the built-in modulation comes back with set_channel once the table is cleared ...
        dec.set_constellation(None)
        dec.set_channel(ChannelSpec("awgn", "qam16"))
        _, llr = dec.generate(SEED, 3, GEN_SIGMA[4], 1000, 70)
        want, M = channel_ref.frames_llr(ChannelSpec("awgn", "qam16"), _bits(W576, 3, 1000, 70)[1], SEED, 3,
                                         GEN_SIGMA[4], 1000)
        assert (np.abs(llr - want) <= 1e-12 * np.maximum(1.0, M)[:, None] + 1e-12 * np.abs(want)).all()
    finally:
        dec.set_harq(None)
        dec.set_rate_match(None)
        dec.set_constellation(None)
        dec.set_channel(None)
    # ... and the reference channel's frames and parity mode after going back
    H = hstd_for(W576)
    u, llr = dec.generate(SEED, 3, 0.8, 1000, 70)
    uo, _, lo = oracle.generate_frames(H, SEED, 3, 0.8, 1000, 70)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
    assert dec.mc_run(SEED, [0.8], 64, 0, 5)[0, 0] == 64
    assert len(dec.frame_order(SEED, 0, 0.8, 0, 64)) == 64
    # n = 7 under bps = 3
    Hb = hstd_for("BCH_7_4_1_strip")
    bch = Decoder(Graph.cached(Hb), 64)
    try:
        bch.set_channel(ChannelSpec("awgn"))
        bch.set_constellation(p8)
        _einval(lambda: bch.generate(SEED, 0, 0.5, 0, 8), "n = 7", "bps = 3", clear)
        _einval(lambda: bch.phys_mc_run(Graph.cached(Hb), SEED, [0.5], 8, 0, 5), "n = 7", "bps = 3")
        bch.set_constellation(TABLES["two"])  # bps = 1 divides everything
        assert np.isfinite(bch.generate(SEED, 0, 0.5, 0, 8)[1]).all()
        bch.set_constellation(None)
        bch.set_channel(None)
        u, llr = bch.generate(SEED, 0, 0.5, 0, 8)
        uo, _, lo = oracle.generate_frames(Hb, SEED, 0, 0.5, 0, 8)
        np.testing.assert_array_equal(u, uo)
        np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
    finally:
        bch.close()
    assert a16.bps == 4


# ------------------------------------------------------- 7. untouched default
def test_without_a_table_nothing_moved(gpu_available):
    """generate() under every existing ChannelSpec (the reference channel and
    the sixteen models), and under a pattern with an interleaver and block
    fading and under a HARQ plan, before and after a table was set, used and
    cleared on the same decoder: bit-identical arrays."""
    dec = _decoder(W576, 128)
    specs = [ChannelSpec()] + [ChannelSpec(model, mod, demap) for model in ("awgn", "rayleigh")
                               for mod in ("bpsk", "qpsk", "qam16", "qam64") for demap in ("exact", "maxlog")]
    rm = RateMatch(tuple(range(288, 576, 12)), ())  # E = 552, a multiple of 1, 2, 4 and 6

    def sweep():
        out = []
        for spec in specs:
            dec.set_channel(spec)
            out.append(dec.generate(SEED, 3, 0.8 if spec.is_reference else GEN_SIGMA[spec.bps], 1000, 70))
        dec.set_channel(ChannelSpec("rayleigh", "qam16"))
        dec.set_rate_match(rm)
        dec.set_interleaver(interleave.random(552, 7))
        dec.set_fading_block(7)
        out.append(dec.generate(SEED, 3, 0.3, 1000, 70))
        dec.set_interleaver(None)
        dec.set_rate_match(None)
        dec.set_harq(HarqPlan.ir(576, 3, 240))
        out.append(dec.generate(SEED, 3, 0.3, 1000, 70))
        dec.set_harq(None)
        dec.set_fading_block(1)
        dec.set_channel(None)
        return out
    try:
        before = sweep()
        assert dec.constellation is None
        for model, demap in SPECS:
            with _under(dec, model, demap, TABLES["rand64"]):
                assert np.isfinite(dec.generate(SEED, 3, 0.15, 1000, 70)[1]).all()  # the table's kernels ran on it
        with _under(dec, "rayleigh", "exact", TABLES["16apsk"], None, None, 5, HarqPlan.ir(576, 3, 240)):
            dec.generate(SEED, 3, 0.3, 1000, 70)
        assert dec.constellation is None
        after = sweep()
    finally:
        dec.set_harq(None)
        dec.set_interleaver(None)
        dec.set_rate_match(None)
        dec.set_fading_block(1)
        dec.set_constellation(None)
        dec.set_channel(None)
    for (ub, lb), (ua, la) in zip(before, after):
        np.testing.assert_array_equal(ub, ua)
        assert lb.tobytes() == la.tobytes()
