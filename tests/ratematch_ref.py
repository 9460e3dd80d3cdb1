"""numpy restatement of the frame source under a rate-matching pattern
(include/ldpc_hip.h, "rate matching") -- a test helper, not a test.

It shares no code with the kernels: the info bits come from the committed CPU
frame source (oracle.generate_frames) and have the shortened positions
cleared; the codeword is re-encoded from H itself ([u, A u mod 2] for
H = [A | I], the running XOR of the info-part syndromes for an IRA graph) and
checked against H; the COMPACTED transmitted bits c[tx] go through the channel
restatement (tests/channel_ref.py, unchanged) as a code of length E, and the
result is scattered back; the columns not sent get +0.0 and -KNOWN_LLR.
"""
import numpy as np
from scipy import sparse

import channel_ref
import oracle
from ldpc_amd.ratematch import KNOWN_LLR


def encode(H, u, ira):
    """Codewords [count, n] of the info words u [count, k] on H = [A | I_m], or
    (ira) H = [H_info | staircase]; H c = 0 asserted."""
    H = sparse.csr_matrix(H)
    m, n = H.shape
    k = n - m
    u = np.asarray(u, np.uint8)
    s = (np.asarray(H[:, :k].astype(np.int64) @ u.T.astype(np.int64)) % 2).T.astype(np.uint8)  # [count, m]
    par = np.bitwise_xor.accumulate(s, axis=1) if ira else s
    c = np.concatenate([u, par], axis=1).astype(np.uint8)
    assert not (np.asarray(H.astype(np.int64) @ c.T.astype(np.int64)) % 2).any(), "H c != 0"
    return c


def bits(H, ira, rm, seed, snr_point, frame0, count):
    """(u, c) of the frames under the pattern: the frame source's info words
    with the shortened positions cleared, and their codewords."""
    u, _, _ = oracle.generate_frames(H, seed, snr_point, 1.0, frame0, count, ira=ira)
    u = u.copy()
    u[:, list(rm.shortened)] = 0
    return u, encode(H, u, ira)


def frames_llr(spec, rm, c, seed, snr_point, sigma, frame0):
    """(llr [count, n], M [count]): the LLRs of the frames frame0 .. whose
    codewords are c, and each frame's largest per-axis metric."""
    c = np.asarray(c, np.uint8)
    count, n = c.shape
    tx = np.array(rm.transmitted(n), np.int64)
    llr = np.empty((count, n), np.float64)
    M = np.empty(count)
    for f in range(count):
        sent, M[f] = channel_ref.frame_llr(spec, c[f, tx], seed, frame0 + f, snr_point, sigma)
        llr[f, tx] = sent
    llr[:, list(rm.punctured)] = 0.0
    llr[:, list(rm.shortened)] = -KNOWN_LLR
    return llr, M
