"""numpy restatement of the frame source's channel models (include/ldpc_hip.h,
"channel models") -- a test helper, not a test.

It is formulated differently from the kernels on purpose: the kernels demap
each axis of a square constellation on its own; this file builds the whole
constellation from a written-out bit -> level table and goes over all 2^bps
complex points of every symbol by brute force.  Only the draws (the Philox
counters, Box-Muller, the fade) are shared, through oracle.philox.

  constellation(bps)            points [2^bps] complex, labels [2^bps, bps]
  frame_llr(spec, c, ...)       LLRs of one frame from its codeword bits c
  frames_llr(spec, c, ...)      the same for consecutive frames, plus the largest
                                per-axis metric M of each frame (the tolerance's scale)
  expected_ber(spec, sigma)     error probability of nearest-point decisions per
                                bit-position class (I/Q merged), from Gaussian tail
                                sums over the decision regions; Rayleigh by quadrature
"""
import functools
import itertools
import math

import numpy as np

import oracle

# the Gray tables of the contract, written out: axis bits (a0, ...) -> level in units of d
AXIS_LEVELS = {
    1: {(0,): -1, (1,): +1},
    2: {(0, 0): -3, (0, 1): -1, (1, 1): +1, (1, 0): +3},
    3: {(0, 0, 0): -7, (0, 0, 1): -5, (0, 1, 1): -3, (0, 1, 0): -1,
        (1, 1, 0): +1, (1, 1, 1): +3, (1, 0, 1): +5, (1, 0, 0): +7},
}
SCALE = {1: 1.0, 2: 1.0 / math.sqrt(2.0), 4: 1.0 / math.sqrt(10.0), 6: 1.0 / math.sqrt(42.0)}  # d by bps


@functools.lru_cache(maxsize=None)
def constellation(bps):
    """(points, labels): point p carries the bits labels[p] (first bps/2 on I,
    the rest on Q); p is the number those bits spell, first bit most significant."""
    labels = np.array(list(itertools.product((0, 1), repeat=bps)), np.uint8)
    d = SCALE[bps]
    if bps == 1:
        pts = np.array([AXIS_LEVELS[1][tuple(b)] * d for b in labels], np.complex128)
    else:
        m = bps // 2
        pts = np.array([complex(AXIS_LEVELS[m][tuple(b[:m])] * d, AXIS_LEVELS[m][tuple(b[m:])] * d) for b in labels])
    pts.setflags(write=False)
    labels.setflags(write=False)
    return pts, labels


def _u52(hi, lo):
    return (float(((int(hi) << 32) | int(lo)) >> 12) + 0.5) * 2.0 ** -52


def _block(seed, F, snr_point, word2):
    return oracle.philox([F & 0xFFFFFFFF, (F >> 32) & 0xFFFFFFFF, word2, ((snr_point << 1) | 1) & 0xFFFFFFFF],
                         (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))


@functools.lru_cache(maxsize=None)
def noise_pairs(seed, F, snr_point, count):
    """[count, 2] N(0,1): row b is the frame source's noise_pair(seed, F, p, b)."""
    out = np.empty((count, 2))
    for b in range(count):
        c = _block(seed, F, snr_point, b)
        r = math.sqrt(-2.0 * math.log(_u52(c[0], c[1])))
        th = 6.283185307179586 * _u52(c[2], c[3])
        out[b] = r * math.cos(th), r * math.sin(th)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def fades(seed, F, snr_point, count):
    """[count] h = sqrt(-log u) of symbols (BPSK: bits) 0 .. count - 1."""
    out = np.empty(count)
    for b in range((count + 1) // 2):
        c = _block(seed, F, snr_point, 0x80000000 | b)
        out[2 * b] = math.sqrt(-math.log(_u52(c[0], c[1])))
        if 2 * b + 1 < count:
            out[2 * b + 1] = math.sqrt(-math.log(_u52(c[2], c[3])))
    out.setflags(write=False)
    return out


def frame_llr(spec, c, seed, F, snr_point, sigma):
    """(llr [n], M): the LLRs of frame F whose codeword bits are c, and the
    largest per-axis metric mu of the frame."""
    c = np.asarray(c, np.uint8)
    n, bps = len(c), spec.bps
    assert n % bps == 0
    S = n // bps
    pts, labels = constellation(bps)
    if bps == 1:
        g = noise_pairs(seed, F, snr_point, (n + 1) // 2).reshape(-1)[:n].astype(np.complex128)
    else:
        gp = noise_pairs(seed, F, snr_point, S)
        g = gp[:, 0] + 1j * gp[:, 1]
    h = fades(seed, F, snr_point, S) if spec.model == "rayleigh" else np.ones(S)
    bits = c.reshape(S, bps)
    sent = bits.astype(np.int64) @ (1 << np.arange(bps - 1, -1, -1))  # the point those bits spell
    y = h * pts[sent] + sigma * g
    diff = y[:, None] - h[:, None] * pts[None, :]  # [S, 2^bps]
    two_s2 = 2.0 * sigma * sigma
    metric = (diff.real ** 2 + diff.imag ** 2) / two_s2
    M = float(max((diff.real ** 2).max(), (diff.imag ** 2).max()) / two_s2)
    llr = np.empty((S, bps))
    for t in range(bps):
        one, zero = metric[:, labels[:, t] == 1], metric[:, labels[:, t] == 0]
        if spec.demap == "maxlog":
            llr[:, t] = zero.min(axis=1) - one.min(axis=1)
        else:
            m1, m0 = one.min(axis=1), zero.min(axis=1)
            llr[:, t] = (np.log(np.exp(-(one - m1[:, None])).sum(axis=1)) - m1) - \
                        (np.log(np.exp(-(zero - m0[:, None])).sum(axis=1)) - m0)
    return llr.reshape(n), M


def frames_llr(spec, c, seed, snr_point, sigma, frame0):
    """(llr [count, n], M [count]) of the frames frame0 .. with codeword bits c [count, n]."""
    out = [frame_llr(spec, row, seed, frame0 + f, snr_point, sigma) for f, row in enumerate(np.asarray(c))]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def bit_classes(bps, n):
    """[n] class of every codeword bit: its position on its axis (a0 = 0, ...)."""
    m = max(bps // 2, 1)
    return (np.arange(n) % bps) % m


def _q(x):
    return 0.5 * math.erfc(x / math.sqrt(2.0))


def _axis_ber(m, d, sigma, h):
    """[m] bit error probabilities of nearest-level decisions on one axis at fade h."""
    table = AXIS_LEVELS[m]
    lab = sorted(table, key=table.get)       # labels in level order
    lev = [table[a] * d * h for a in lab]    # received levels, ascending
    err = np.zeros(m)
    for i, xi in enumerate(lev):
        for k in range(len(lev)):
            lo = -math.inf if k == 0 else 0.5 * (lev[k - 1] + lev[k])
            hi = math.inf if k == len(lev) - 1 else 0.5 * (lev[k] + lev[k + 1])
            p = _q((lo - xi) / sigma) - _q((hi - xi) / sigma)
            for t in range(m):
                if lab[i][t] != lab[k][t]:
                    err[t] += p
    return err / len(lev)


def expected_ber(spec, sigma, steps=4000, hmax=8.0):
    """[classes] error probability of nearest-point decisions per bit-position
    class.  Rayleigh: the integral over h with weight 2 h exp(-h^2), Simpson's
    rule on [0, hmax] (the weight beyond hmax = 8 is e^-64)."""
    m, d = max(spec.bps // 2, 1), SCALE[spec.bps]
    if spec.model != "rayleigh":
        return _axis_ber(m, d, sigma, 1.0)
    hs = np.linspace(0.0, hmax, steps + 1)
    w = np.ones(steps + 1)
    w[1:-1:2], w[2:-1:2] = 4.0, 2.0
    w *= (hmax / steps) / 3.0
    vals = np.array([_axis_ber(m, d, sigma, h) if h > 0.0 else np.full(m, 0.5) for h in hs])
    return (vals * (w * 2.0 * hs * np.exp(-hs * hs))[:, None]).sum(axis=0)
