"""The bit-flipping decoders without a GPU: the numpy restatement
(tests/bitflip_ref.py) against an independent integer majority-rule loop and
its own invariants, the sliced kernel's threshold rule and bit-plane counting
in numpy, and the refusals of the Python layer and the command line."""
import numpy as np
import pytest

import bitflip_ref
import synth_graphs
from ldpc_amd import montecarlo as mc
from ldpc_amd.device import bitflip_args

T = 10


def _hard(llr):
    return (-(np.asarray(llr).astype(np.float32)) < 0).astype(np.int64)


def _majority(H, llr, T):
    """Plain integer majority flipping, frame by frame: flip bit j when more
    than half of its checks fail (2 u_j > d_j)."""
    Hd = np.asarray(H.todense()).astype(np.int64)
    d = Hd.sum(axis=0)
    z, conv = [], []
    for x in _hard(llr):
        b, cv = x.copy(), -1
        for it in range(T):
            s = Hd @ b % 2
            if s.any():
                b = b ^ (2 * (s @ Hd) > d)
                s = Hd @ b % 2
            if not s.any():
                cv = it
                break
        z.append(b ^ 1)
        conv.append(cv)
    return np.array(z, np.uint8), np.array(conv, np.int32)


@pytest.mark.parametrize("name", ["ragged", "widecol"])
def test_restatement_is_the_majority_rule_at_zero_weight_and_theta(name):
    H = synth_graphs.graph(name)
    llr = synth_graphs.noisy_frames(H.shape[1], 0.5, 70, 1234)
    r = bitflip_ref.decode(H, llr, T)
    z, conv = _majority(H, llr, T)
    np.testing.assert_array_equal(r["z"], z)
    np.testing.assert_array_equal(r["conv"], conv)
    assert 3 <= (conv >= 0).sum() <= 67


@pytest.mark.parametrize("w,theta", [(0.0, 0.0), (0.25, 0.0), (0.0, -1.0), (0.0, 0.5)])
def test_restatement_invariants(w, theta):
    H = synth_graphs.graph("ragged")
    llr = synth_graphs.noisy_frames(H.shape[1], 0.5, 70, 1234)
    r = bitflip_ref.decode(H, llr, T, w, theta)
    ok = r["conv"] >= 0
    b = (r["z"] ^ 1).astype(np.int64)
    syn = (H.astype(np.int64) @ b.T).T % 2
    np.testing.assert_array_equal(r["synw"], syn.sum(axis=1))
    assert (r["synw"][ok] == 0).all() and (r["synw"][~ok] > 0).all()
    np.testing.assert_array_equal(r["status"], (~ok).astype(np.int32))
    np.testing.assert_array_equal(r["iters"], np.where(ok, r["conv"] + 1, T))
    assert r["z"].dtype == np.uint8 and r["conv"].dtype == np.int32 and r["synw"].dtype == np.int32


def test_a_codeword_at_input_has_conv_zero_and_no_flips():
    H = synth_graphs.graph("widecol")
    n = H.shape[1]
    llr = np.full((2, n), -3.0)  # the all-zero codeword, bit 0 <-> llr < 0 (Lam > 0)
    llr[1, ::3] = -0.0           # Lam = +0.0 is bit 0 too
    for w, theta in ((0.0, 0.0), (0.5, 0.0), (0.0, -1.0)):
        r = bitflip_ref.decode(H, llr, T, w, theta)
        assert (r["conv"] == 0).all() and (r["iters"] == 1).all() and (r["synw"] == 0).all()
        np.testing.assert_array_equal(r["z"], _hard(llr) ^ 1)


def test_zero_weight_ignores_non_finite_llr():
    H = synth_graphs.graph("ragged")
    llr = synth_graphs.noisy_frames(H.shape[1], 0.5, 8, 1234)
    big = llr.copy()
    big[:, 5] = np.where(big[:, 5] < 0, -np.inf, np.inf)
    a, b = bitflip_ref.decode(H, llr, T), bitflip_ref.decode(H, big, T)
    for key in a:
        np.testing.assert_array_equal(a[key], b[key], err_msg=key)


@pytest.mark.parametrize("theta", [0.0, -1.0, 0.5, 100.0, -100.0])
def test_threshold_table_is_the_fp32_comparison(theta):
    t = bitflip_ref.thresholds(theta, 63)
    th = np.float32(theta)
    for d in range(64):
        u = np.arange(d + 1)
        np.testing.assert_array_equal(u >= t[d], (d - 2 * u).astype(np.float32) < th, err_msg=f"d={d}")
        assert 0 <= t[d] <= d + 1


def _sliced(H, llr, T, theta):
    """The sliced kernel's algorithm on 64-bit words in numpy: bit f of word j
    is frame f; u_j in bit planes (ripple half-adder per row word), compared
    with t(d_j) from the top plane down.  Returns (z, conv) of up to 64 frames."""
    H = H.tocsr()
    Hc = H.tocsc()
    m, n = H.shape
    d = np.diff(Hc.indptr)
    t = bitflip_ref.thresholds(theta, int(max(d.max(), 1)))
    planes = int(d.max()).bit_length()
    cnt = len(llr)
    b = _hard(llr)
    one = np.uint64(1)
    bw = np.zeros(n, np.uint64)
    for f in range(cnt):
        bw |= b[f].astype(np.uint64) << np.uint64(f)
    full = np.uint64(0xFFFFFFFFFFFFFFFF)

    def syndrome():
        sw = np.zeros(m, np.uint64)
        for r in range(m):
            for c in H.indices[H.indptr[r]:H.indptr[r + 1]]:
                sw[r] ^= bw[c]
        return sw, np.bitwise_or.reduce(sw) if m else np.uint64(0)

    sw, bad = syndrome()
    active = full if cnt == 64 else (one << np.uint64(cnt)) - one
    conv = np.full(cnt, -1, np.int32)
    for it in range(T):
        run = active & bad
        if run:
            for j in range(n):
                if t[d[j]] > d[j]:
                    continue
                c = [np.uint64(0)] * planes
                for r in Hc.indices[Hc.indptr[j]:Hc.indptr[j + 1]]:
                    carry = sw[r]
                    for i in range(planes):
                        c[i], carry = c[i] ^ carry, c[i] & carry
                ge, eq = np.uint64(0), full
                for i in reversed(range(planes)):
                    tm = full if (int(t[d[j]]) >> i) & 1 else np.uint64(0)
                    ge |= eq & c[i] & ~tm
                    eq &= ~(c[i] ^ tm)
                bw[j] ^= (ge | eq) & run
            sw, bad = syndrome()
        done = active & ~bad
        for f in range(cnt):
            if (done >> np.uint64(f)) & one:
                conv[f] = it
        active &= bad
        if not active:
            break
    z = np.array([[1 - int((bw[j] >> np.uint64(f)) & one) for j in range(n)] for f in range(cnt)], np.uint8)
    return z, conv


@pytest.mark.parametrize("name,theta", [("ragged", 0.0), ("ragged", 0.5), ("widecol", -1.0)])
def test_bit_sliced_counting_equals_the_restatement(name, theta):
    H = synth_graphs.graph(name)
    llr = synth_graphs.noisy_frames(H.shape[1], 0.5, 70, 1234)[:40]  # a ragged tile
    r = bitflip_ref.decode(H, llr, 5, 0.0, theta)
    z, conv = _sliced(H, llr, 5, theta)
    np.testing.assert_array_equal(z, r["z"])
    np.testing.assert_array_equal(conv, r["conv"])


def test_bitflip_args_refuse_before_any_device_call():
    assert bitflip_args() == (0.0, 0.0) and bitflip_args(0.5, -1) == (0.5, -1.0)
    for w, th in ((-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (1e39, 0.0), (0.0, float("nan")),
                  (0.0, float("inf")), ("x", 0.0)):
        with pytest.raises(ValueError):
            bitflip_args(w, th)


def test_simulate_refuses_before_any_device_call():
    snrs = [0.0]
    for kw in (dict(mode="parity"), dict(mode="physical", cn_rule="nms"), dict(mode="physical", qbits=6, cn_rule="nms"),
               dict(mode="physical", schedule="layered", cn_rule="nms"), dict(mode="physical", nllr=True),
               dict(mode="physical", bf_weight=-1.0), dict(mode="physical", bf_weight=float("nan")),
               dict(mode="physical", bf_weight=float("inf")), dict(mode="physical", bf_theta=float("nan"))):
        with pytest.raises(ValueError):
            mc.simulate("wimax_576_0.5", snrs, 4, 5, decoder="bitflipping", **kw)
    with pytest.raises(ValueError):
        mc.simulate("wimax_576_0.5", snrs, 4, 5, mode="physical", decoder="gallager")
    with pytest.raises(ValueError):  # the parameters without the decoder
        mc.simulate("wimax_576_0.5", snrs, 4, 5, mode="physical", bf_weight=0.5)


def test_decoder_type_strings():
    assert mc.bitflip_decoder_type() == "bitflipping" and mc.bitflip_decoder_type(0.0) == "bitflipping"
    assert mc.bitflip_decoder_type(0.5) == "bitflipping-gd"
    assert mc.decoder_type("spa", "flooding") == "sumproduct"  # positional, unchanged


def test_cli_options(capsys):
    a = mc.parse_args(["--matrix", "x"])
    assert (a.decoder, a.bf_weight, a.bf_theta) == ("sumproduct", 0.0, 0.0)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--decoder", "bitflipping"])
    assert (a.decoder, a.bf_weight, a.bf_theta) == ("bitflipping", 0.0, 0.0)
    a = mc.parse_args(["--matrix", "x", "--mode", "physical", "--decoder", "bitflipping", "--bf-weight", "0.5",
                       "--bf-theta", "-1", "--channel", "awgn", "--modulation", "qam16", "--stats-json", "s.json"])
    assert (a.bf_weight, a.bf_theta) == (0.5, -1.0)
    bf = ["--mode", "physical", "--decoder", "bitflipping"]
    for argv in (["--decoder", "bitflipping"],  # parity mode
                 ["--mode", "physical", "--bf-weight", "0.5"], ["--mode", "physical", "--bf-theta", "1"],
                 bf + ["--cn-rule", "nms"], bf + ["--cn-rule", "nms", "--qbits", "6"],
                 bf + ["--cn-rule", "nms", "--schedule", "layered"], bf + ["--normalized-llr"],
                 bf + ["--bf-weight", "-1"], bf + ["--bf-weight", "nan"], bf + ["--bf-weight", "inf"],
                 bf + ["--bf-theta", "nan"], ["--mode", "physical", "--decoder", "gallager"]):
        with pytest.raises(SystemExit) as e:
            mc.parse_args(["--matrix", "x"] + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
