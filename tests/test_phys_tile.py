"""Physical mode with HBM-resident state + the IRA (DVB-S2-profile) frame
source -- BASELINE config 5.  OUR design (no reference parity by
construction): the HBM tile path must be
BIT-IDENTICAL to the LDS path (same phi, same operation order), and both are
checked against the CPU restatement (oracle/phys_oracle.c); the IRA generator
against oracle/channel_oracle.c (ira=1)."""
import collections

import numpy as np
import pytest

import ldpc_amd
import oracle
from ldpc_amd import ira
from ldpc_amd import montecarlo as mc

SEED = 20260213


@pytest.fixture(scope="module")
def dvbs2():
    return ira.dvbs2_profile_matrix()


def test_dvbs2_profile_structure(dvbs2):
    """n=64800 r1/2 normal frame: DVB-S2's rate-1/2 degree profile exactly."""
    H = dvbs2
    assert H.shape == (32400, 64800) and H.nnz == 226799
    assert collections.Counter(np.diff(H.indptr).tolist()) == {7: 32399, 6: 1}
    cols = collections.Counter(np.diff(H.tocsc().indptr).tolist())
    assert cols == {8: 12960, 3: 19440, 2: 32399, 1: 1}
    assert ira.is_ira(H)
    u = np.random.default_rng(3).integers(0, 2, size=(4, 32400))
    c = ira.encode(H, u)
    assert not ((H @ c.T.astype(np.int64)) % 2).any()


def test_small_ira_and_alist_round_trip(tmp_path):
    from ldpc_amd.alist import read_parity_check_matrix, write_alist
    H = ira.small_ira_matrix()
    assert ira.is_ira(H) and not ira.is_ira(ldpc_amd.load_committed_code("wimax_576_0.5")._h_std)
    write_alist(H, tmp_path / "ira.alist")
    back = read_parity_check_matrix(str(tmp_path / "ira.alist"))
    assert (back != H).nnz == 0


def test_oracle_ira_frames_are_codewords():
    H = ira.small_ira_matrix()
    u, c, llr = oracle.generate_frames(H, SEED, 1, mc.sigma_for_snr(0.0), 100, 32, ira=True)
    np.testing.assert_array_equal(ira.encode(H, u), c)
    # same info bits and noise draws as the [A|I] generator: only parities differ
    Hs = ldpc_amd.load_committed_code("wimax_576_0.5")._h_std
    u2, _, _ = oracle.generate_frames(Hs, SEED, 1, mc.sigma_for_snr(0.0), 100, 32)
    np.testing.assert_array_equal(u[:, :288], u2[:, :288])
    r = oracle.phys_decode(H, llr, 30)
    assert (r["status"] == 0).all()
    np.testing.assert_array_equal(r["z"] ^ 1, c)


# ------------------------------------------------------------------ GPU
def _graph(H):
    from ldpc_amd.device import Graph
    return Graph.cached(H)


@pytest.mark.gpu
@pytest.mark.parametrize("name,snr,B", [("wimax_576_0.5", -2.5, 192), ("wimax_2304_0.5", -2.5, 96),
                                         ("wimax_2304_0.75A", -1.0, 96), ("wimax_576_0.5", 0.0, 192)])
def test_hbm_path_bit_identical_to_lds(gpu_available, name, snr, B):
    """The 0 dB case pins the HBM path's early syndrome (phys_tile.hip's
    phys_tile_syn_kernel, then phys_tile_state.hip's phys_tile_exit_kernel, the
    exit both tile families share, after VN(1) and VN(2): conv = it, iters =
    it + 1) to the LDS kernel frame by frame."""
    from ldpc_amd.device import phys_decode
    edd = ldpc_amd.load_committed_code(name)
    Hp = edd.physical_matrix()
    _, _, llr = oracle.generate_frames(edd._h_std, SEED, 5, mc.sigma_for_snr(snr), 0, B)
    g = _graph(Hp)
    a = phys_decode(g, llr, 50, post=True)
    b = phys_decode(g, llr, 50, post=True, hbm=True)
    if name == "wimax_576_0.5" and snr < 0:
        assert 0 < (a.status == 0).sum() < B  # a mix of outcomes (waterfall)
    if snr >= 0:  # frames that stop at the early syndrome after VN(1) / VN(2)
        assert np.isin(b.iters, (2, 3)).sum() > 0, np.bincount(b.iters)
    for key in ("z", "conv", "status", "iters"):
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)
    np.testing.assert_array_equal(a.post.view(np.uint32), b.post.view(np.uint32))


@pytest.mark.gpu
def test_phys_mc_hbm_counters_equal_lds(gpu_available, monkeypatch):
    from ldpc_amd.device import Decoder
    edd = ldpc_amd.load_committed_code("wimax_576_0.5")
    dec = Decoder(_graph(edd._h_std), 1024)
    gp = _graph(edd.physical_matrix())
    sig = [mc.sigma_for_snr(s) for s in (-3.0, -2.5, 0.0)]
    a = dec.phys_mc_run(gp, SEED, sig, 2000, 64, 50)
    dec.profile(True)
    b = dec.phys_mc_run(gp, SEED, sig, 2000, 64, 50, hbm=True)
    p = dec.profile_read()
    dec.profile(False)
    np.testing.assert_array_equal(a, b)
    # the HBM path compacted its running frames (round 5: the finished frames
    # are counted before the move, so more count launches than chunks)
    chunks = 3 * 2
    assert p["count"][1] > chunks, p["count"]
    monkeypatch.setenv("LDPC_PHYS_COMPACT", "0")  # the switch (A/B, diagnosis): same counters
    np.testing.assert_array_equal(dec.phys_mc_run(gp, SEED, sig, 2000, 64, 50, hbm=True), a)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["small", "dvbs2"])
def test_ira_generator_matches_restatement(gpu_available, dvbs2, which):
    from ldpc_amd.device import Decoder
    H = ira.small_ira_matrix() if which == "small" else dvbs2
    B = 200 if which == "small" else 64
    dec = Decoder(_graph(H), B)
    sigma = mc.sigma_for_snr(-1.0)
    u, llr = dec.generate(SEED, 2, sigma, 777, B)
    uo, co, lo = oracle.generate_frames(H, SEED, 2, sigma, 777, B, ira=True)
    np.testing.assert_array_equal(u, uo)
    np.testing.assert_allclose(llr, lo, rtol=1e-12, atol=1e-12)
    assert not ((H @ co.T.astype(np.int64)) % 2).any()


@pytest.mark.gpu
@pytest.mark.parametrize("snr", [-2.75, 1.0])
def test_dvbs2_decode_matches_restatement(gpu_available, dvbs2, snr):
    from ldpc_amd.device import phys_decode
    _, c, llr = oracle.generate_frames(dvbs2, SEED, 0, mc.sigma_for_snr(snr), 0, 48, ira=True)
    g = phys_decode(_graph(dvbs2), llr, 50, post=True)
    o = oracle.phys_decode(dvbs2, llr, 50)
    # hardware exp/log vs libm expf/logf: a marginal frame may flip, never many
    same = (g.z == o["z"]).all(axis=1) & (g.conv == o["conv"])
    assert same.mean() >= 0.9, same.mean()
    agree = same.nonzero()[0]
    gp, op = g.post[agree], o["post"][agree]
    # Saturated posteriors: a check whose inputs are all reliable has S = sum
    # phi ~ 1e-7, and phi(S) = log(2/S) turns the ~1e-7 ABSOLUTE error of
    # hardware vs libm exp/log near 1 into a few % of a ~15 message.  Decision
    # irrelevant (|L| >> 0); moderate posteriors must agree tightly.
    mod = np.abs(op) < 8.0
    np.testing.assert_allclose(gp[mod], op[mod], rtol=2e-3, atol=2e-3)
    np.testing.assert_allclose(gp[~mod], op[~mod], rtol=0.1)
    assert (np.sign(gp) == np.sign(op)).all()
    if snr > 0:
        assert (g.status == 0).all()
        np.testing.assert_array_equal(g.z ^ 1, c)


@pytest.mark.gpu
def test_dvbs2_mc_counters(gpu_available, dvbs2):
    """Config 5 path: IRA frames generated on the device, HBM-resident decode."""
    from ldpc_amd.device import Decoder
    g = _graph(dvbs2)
    dec = Decoder(g, 256)
    sig = [mc.sigma_for_snr(s) for s in (-3.5, -2.75, 1.0)]
    ctr = dec.phys_mc_run(g, SEED, sig, 320, 0, 50)  # two chunks, the second ragged
    for c in ctr:
        frames, failed, err, sconv, nconv, _, iters = (int(x) for x in c)
        assert frames == 320 and failed == frames - nconv
        assert iters == sconv + nconv + failed * 50
        assert (err > 0) == (failed > 0)
    assert ctr[0, 1] == 320 and ctr[2, 1] == 0  # below / above the waterfall
    # counters == restatement on the same device-generated frames
    u, llr = Decoder(g, 64).generate(SEED, 1, sig[1], 0, 64)
    o = oracle.phys_decode(dvbs2, llr, 50)
    want = oracle.main_counters(u, o["z"], o["status"], o["conv"], iters=o["iters"])
    got = dec.phys_mc_run(g, SEED, sig, 64, 0, 50)[1]
    assert abs(int(got[1]) - int(want[1])) <= 3
