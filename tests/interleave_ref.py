"""numpy restatement of the frame source under a bit interleaver and block
fading (include/ldpc_hip.h, "bit interleaver and block fading") -- a test
helper, not a test.

It shares no code with the kernels.  The bits are ratematch_ref.bits (the
interleaver changes no bit).  The INTERLEAVED transmitted bits c[tx[pi]] are
taken as a code of length E and go, symbol by symbol, over the whole
constellation by brute force, as channel_ref.frame_llr does, with
channel_ref's constellation, noise_pairs and fades; under block fading the
fades are fades(...)[:nblocks], each repeated block_len times.  The LLRs are
scattered back to the columns tx[pi]; the columns not sent are filled as
ratematch_ref fills them.  With the identity (or no interleaver) and block_len
1 every operation is channel_ref.frame_llr's, on the same numbers, so the
result equals ratematch_ref.frames_llr exactly
(tests/test_interleave_host.py).
"""
import numpy as np

import channel_ref
from ldpc_amd.ratematch import KNOWN_LLR, RateMatch


def columns(rm, perm, n):
    """col[t] = tx[pi[t]]: the column of transmitted position t (perm None: tx)."""
    tx = np.array((rm or RateMatch()).transmitted(n), np.int64)
    if perm is None:
        return tx
    perm = np.asarray(perm, np.int64)
    assert sorted(perm.tolist()) == list(range(len(tx))), "not a permutation of 0 .. E-1"
    return tx[perm]


def block_fades(seed, F, snr_point, S, block_len):
    """[S] the fade of every symbol (BPSK: position): index floor(s / block_len)."""
    nblocks = -(-S // block_len)
    return np.repeat(channel_ref.fades(seed, F, snr_point, nblocks), block_len)[:S]


def sent_llr(spec, c, seed, F, snr_point, sigma, block_len=1):
    """(llr [E], M) of frame F whose E transmitted bits, in transmission
    order, are c; M the largest per-axis metric (the tolerance's scale)."""
    c = np.asarray(c, np.uint8)
    n, bps = len(c), spec.bps
    assert n % bps == 0
    S = n // bps
    pts, labels = channel_ref.constellation(bps)
    if bps == 1:
        g = channel_ref.noise_pairs(seed, F, snr_point, (n + 1) // 2).reshape(-1)[:n].astype(np.complex128)
    else:
        gp = channel_ref.noise_pairs(seed, F, snr_point, S)
        g = gp[:, 0] + 1j * gp[:, 1]
    h = block_fades(seed, F, snr_point, S, block_len) if spec.model == "rayleigh" else np.ones(S)
    bits = c.reshape(S, bps)
    sent = bits.astype(np.int64) @ (1 << np.arange(bps - 1, -1, -1))
    y = h * pts[sent] + sigma * g
    diff = y[:, None] - h[:, None] * pts[None, :]
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


def frames_llr(spec, rm, perm, block_len, c, seed, snr_point, sigma, frame0):
    """(llr [count, n], M [count]) of the frames frame0 .. whose codewords are
    c, under the pattern rm (None: none), the interleaver perm (None: none) and
    the coherence length block_len."""
    rm = rm or RateMatch()
    c = np.asarray(c, np.uint8)
    count, n = c.shape
    col = columns(rm, perm, n)
    llr = np.empty((count, n), np.float64)
    M = np.empty(count)
    for f in range(count):
        sent, M[f] = sent_llr(spec, c[f, col], seed, frame0 + f, snr_point, sigma, block_len)
        llr[f, col] = sent
    llr[:, list(rm.punctured)] = 0.0
    llr[:, list(rm.shortened)] = -KNOWN_LLR
    return llr, M
