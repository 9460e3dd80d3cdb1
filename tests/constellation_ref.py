"""numpy restatement of the frame source under a constellation table
(include/ldpc_hip.h, "constellations") -- a test helper, not a test.

It is formulated from the contract and shares only the draws
(channel_ref.noise_pairs, channel_ref.fades) with existing code: the built-in
tables are written out again here, every symbol is demapped by brute force
over all 2^bps points with scipy's logsumexp, and a pattern, an interleaver or
a HARQ plan is nothing but "the list of columns in air order, per
transmission".

  psk8(), apsk16(gamma)     the built-in tables, written out
  frame_llr(points, ...)    LLRs of one transmission from its bits in air order
  compose(points, ...)      a frame from its codeword and the transmissions'
                            column lists, with the per-column tolerance
  frames(points, ...)       the same for consecutive frames
  expected_ber(points, s)   AWGN error probability of nearest-point decisions
                            per bit position
"""
import math

import numpy as np
from scipy.special import logsumexp, ndtr

import channel_ref

KNOWN_LLR = 1.0e4                    # LDPC_RM_KNOWN_LLR
SEED_STEP = 0x9E3779B97F4A7C15       # seed_r = seed + r SEED_STEP mod 2^64
ROTATE = 0.37                        # expected_ber: radians, a multiple of no pi / 24


def psk8():
    """Unit circle; label a0a1a2 -> B by the Gray decoding rule b0 = a0,
    b_i = b_(i-1) xor a_i; angle (2B + 1) pi / 8."""
    pts = np.empty(8, np.complex128)
    for a0 in (0, 1):
        for a1 in (0, 1):
            for a2 in (0, 1):
                b0, b1 = a0, a0 ^ a1
                b2 = b1 ^ a2
                B = 4 * b0 + 2 * b1 + b2
                ang = (2 * B + 1) * math.pi / 8.0
                pts[4 * a0 + 2 * a1 + a2] = complex(math.cos(ang), math.sin(ang))
    return pts


def apsk16(gamma=3.15):
    """4 + 12 points, gamma = R2 / R1; first quadrant by a0a1, a2 negates the
    real part, a3 the imaginary part."""
    r1 = math.sqrt(16.0 / (4.0 + 12.0 * gamma * gamma))
    r2 = gamma * r1
    first = {(0, 0): (r2, math.pi / 4.0), (0, 1): (r2, math.pi / 12.0), (1, 0): (r2, 5.0 * math.pi / 12.0),
             (1, 1): (r1, math.pi / 4.0)}
    pts = np.empty(16, np.complex128)
    for (a0, a1), (r, ang) in first.items():
        for a2 in (0, 1):
            for a3 in (0, 1):
                re, im = r * math.cos(ang), r * math.sin(ang)
                pts[8 * a0 + 4 * a1 + 2 * a2 + a3] = complex(-re if a2 else re, -im if a3 else im)
    return pts


def label_bits(bps):
    """[2^bps, bps]: bit t of label a, the first bit the most significant."""
    a = np.arange(1 << bps)
    return np.array([(a >> (bps - 1 - t)) & 1 for t in range(bps)], np.uint8).T


def _bps(points):
    bps = len(points).bit_length() - 1
    assert len(points) == 1 << bps and bps >= 1
    return bps


def frame_llr(points, model, demap, bits_in_air_order, seed, F, p, sigma, fade_block=1):
    """(llr [E], M): the LLRs of the E positions of one transmission of frame F,
    in air order, and the transmission's largest per-axis metric."""
    points = np.asarray(points, np.complex128)
    bps = _bps(points)
    bits = np.asarray(bits_in_air_order, np.uint8)
    E = len(bits)
    assert E % bps == 0 and E > 0
    S = E // bps
    lab = label_bits(bps)
    sent = bits.reshape(S, bps).astype(np.int64) @ (1 << np.arange(bps - 1, -1, -1))
    gp = channel_ref.noise_pairs(seed, F, p, S)
    if model == "rayleigh":
        idx = np.arange(S) // int(fade_block)
        h = channel_ref.fades(seed, F, p, int(idx.max()) + 1)[idx]
    else:
        assert model == "awgn" and fade_block == 1
        h = np.ones(S)
    y = h * points[sent] + sigma * (gp[:, 0] + 1j * gp[:, 1])
    diff = y[:, None] - h[:, None] * points[None, :]
    two_s2 = 2.0 * sigma * sigma
    mu = (diff.real ** 2 + diff.imag ** 2) / two_s2
    M = float(max((diff.real ** 2).max(), (diff.imag ** 2).max()) / two_s2)
    llr = np.empty((S, bps))
    for t in range(bps):
        one, zero = mu[:, lab[:, t] == 1], mu[:, lab[:, t] == 0]
        if demap == "maxlog":
            llr[:, t] = zero.min(axis=1) - one.min(axis=1)
        else:
            assert demap == "exact"
            llr[:, t] = logsumexp(-one, axis=1) - logsumexp(-zero, axis=1)
    return llr.reshape(E), M


def tx_seed(seed, r):
    return (int(seed) + r * SEED_STEP) % (1 << 64)


def compose(points, model, demap, c, tx_lists, seed, F, p, sigma, fade_block=1, shortened=()):
    """(llr [n], bound [n]) of frame F with codeword c: llr starts at +0.0 and
    takes one fp64 addition per transmission that carries a column (a pattern
    or an interleaver is one transmission: tx_lists = [columns in air order]);
    shortened columns are -KNOWN_LLR.  bound is the project's per-transmission
    tolerance 1e-12 max(1, M_r) + 1e-12 |llr_r[j]| summed over the
    transmissions that carry column j (tests/harq_ref.py)."""
    c = np.asarray(c, np.uint8)
    llr = np.zeros(len(c))
    bound = np.zeros(len(c))
    for r, cols in enumerate(tx_lists):
        cols = np.asarray(cols, np.int64)
        assert len(set(cols.tolist())) == len(cols) and not set(cols.tolist()) & set(shortened)
        sent, M = frame_llr(points, model, demap, c[cols], tx_seed(seed, r), F, p, sigma, fade_block)
        llr[cols] = llr[cols] + sent
        bound[cols] += 1e-12 * max(1.0, M) + 1e-12 * np.abs(sent)
    llr[list(shortened)] = -KNOWN_LLR
    return llr, bound


def frames(points, model, demap, c, tx_lists, seed, p, sigma, frame0, fade_block=1, shortened=()):
    """(llr [count, n], bound [count, n]) of the frames frame0 .. with codewords
    c [count, n]; tx_lists None: every column once, in column order."""
    c = np.asarray(c, np.uint8)
    if tx_lists is None:
        tx_lists = [np.arange(c.shape[1])]
    out = [compose(points, model, demap, row, tx_lists, seed, frame0 + f, p, sigma, fade_block, shortened)
           for f, row in enumerate(c)]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def expected_ber(points, sigma, rows=400, span=6.0):
    """[bps] AWGN error probability of nearest-point decisions per bit position:
    the zero-mean Gaussian of per-axis standard deviation sigma around every
    sent point, integrated over the decision regions of the points whose label
    differs in that bit.  Quadrature on `rows` lines Q = const out to +-span
    sigma around the sent point (midpoint rule); along each line the regions
    are intervals of I, found exactly as the upper envelope of the lines
    2 I x_i,I - |x_i|^2 + 2 Q x_i,Q, and the Gaussian over an interval is a
    difference of two normal distribution functions.  A 400 x 400 grid of cells
    classified by their centres would misplace every region boundary by up to
    half a cell, 1.5 % of sigma, too much for the 1e-3 the tests ask of this
    function; the lines remove that error in one of the two dimensions.  The
    integrand of the other is continuous as long as no boundary runs along a
    line Q = const, so the table is first turned by ROTATE, an angle that no
    table here has a boundary at: the noise is circularly symmetric and the
    error rates do not change.  (Doubling `rows` then moves the result by 1e-5
    of itself for the built-in tables and for 16-QAM.)"""
    pts = np.asarray(points, np.complex128) * complex(math.cos(ROTATE), math.sin(ROTATE))
    bps = _bps(pts)
    lab = label_bits(bps)
    P = len(pts)
    xi, xq = pts.real, pts.imag
    # breakpoints of the envelope: where two lines of different slope cross
    ii, jj = np.triu_indices(P, 1)
    keep = xi[ii] != xi[jj]
    ii, jj = ii[keep], jj[keep]
    step = 2.0 * span * sigma / rows
    err = np.zeros(bps)
    for s in range(P):
        q = xq[s] + (np.arange(rows) + 0.5) * step - span * sigma           # [rows]
        wq = (ndtr((q + 0.5 * step - xq[s]) / sigma) - ndtr((q - 0.5 * step - xq[s]) / sigma))
        off = -(xi ** 2)[None, :] - (q[:, None] - xq[None, :]) ** 2 + (q ** 2)[:, None]  # [rows, P]: -|y - x_i|^2 + I^2 at I = 0
        slope = 2.0 * xi                                                     # d/dI of -|y - x_i|^2 + I^2
        if len(ii):
            br = (off[:, jj] - off[:, ii]) / (slope[ii] - slope[jj])[None, :]
            br = np.sort(br, axis=1)
        else:
            br = np.empty((rows, 0))
        edges = np.concatenate([np.full((rows, 1), -np.inf), br, np.full((rows, 1), np.inf)], axis=1)
        lo, hi = edges[:, :-1], edges[:, 1:]
        mid = np.where(np.isinf(lo), hi - 1.0, np.where(np.isinf(hi), lo + 1.0, 0.5 * (lo + hi)))
        if edges.shape[1] == 2:
            mid = np.zeros((rows, 1))
        win = np.argmax(off[:, None, :] + mid[:, :, None] * slope[None, None, :], axis=2)  # [rows, intervals]
        wi = ndtr((hi - xi[s]) / sigma) - ndtr((lo - xi[s]) / sigma)
        w = wi * wq[:, None]
        for t in range(bps):
            err[t] += w[lab[win, t] != lab[s, t]].sum()
    return err / P
