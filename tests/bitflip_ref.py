"""numpy fp32 restatement of physical mode's bit-flipping decoders (DESIGN.md
"Physical mode: bit-flipping decoders"; include/ldpc_hip.h ldpc_bf_decode).
A helper module, not a test.

Parallel gradient-descent bit flipping with parameters weight w >= 0 and
theta; w = 0 is plain hard-decision flipping, and with theta = 0 the majority
rule.  Every step is one fp32 operation, so the GPU kernels (built without FMA
contraction) must reproduce it bit for bit:
  Lam = -(float)llr,  b = (Lam < 0)           (-0.0 gives bit 0)
  iteration it = 0 .. T-1:
      s_r = XOR of b over row r
      if any s_r:  u_j = sum of s over column j's rows, d_j its degree,
                   c_j = -Lam_j if b_j else Lam_j,
                   Delta_j = fl(fl(w c_j) + (float)(d_j - 2 u_j))
                             ((float)(d_j - 2 u_j) alone when w == 0),
                   every j with Delta_j < theta flips, all from the same s;
                   s is recomputed
      if no s_r:   conv = it, stop
  z = b ^ 1, status = (conv < 0), iters = conv + 1 or T, synw = sum of s at exit.
Frames are vectorised; a frame that has converged is left alone.
"""
import numpy as np
from scipy import sparse


def thresholds(theta, max_deg=63):
    """t [max_deg + 1]: for a column of degree d the smallest u in 0..d with
    (float)(d - 2u) < theta in fp32, d + 1 if there is none.  With w == 0 a
    column flips iff u >= t[d]."""
    th = np.float32(theta)
    t = np.empty(max_deg + 1, np.int64)
    for d in range(max_deg + 1):
        t[d] = d + 1
        for u in range(d + 1):
            if np.float32(d - 2 * u) < th:
                t[d] = u
                break
    return t


def decode(H, llr, T, weight=0.0, theta=0.0):
    """dict(z, conv, status, iters, synw) as ldpc_amd.device.bitflip_decode returns them."""
    H = sparse.csr_matrix(H).astype(np.int32)
    Ht = sparse.csr_matrix(H.T)
    w, th = np.float32(weight), np.float32(theta)
    assert np.isfinite(w) and w >= 0 and np.isfinite(th)
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    B = llr.shape[0]
    d = np.asarray(H.sum(axis=0)).ravel().astype(np.int32)
    with np.errstate(over="ignore"):
        Lam = -(llr.astype(np.float32))
    b = Lam < np.float32(0.0)
    conv = np.full(B, -1, np.int32)

    def syndrome(bits):
        return (np.asarray((H @ bits.T.astype(np.int32)).T) & 1).astype(np.int32)

    s = syndrome(b)
    act = np.arange(B)  # frames still running
    for it in range(int(T)):
        bad = s[act].any(axis=1)
        run = act[bad]
        if len(run):
            u = np.asarray((Ht @ s[run].T).T).astype(np.int32)
            delta = (d[None, :] - 2 * u).astype(np.float32)
            if w != 0:
                with np.errstate(invalid="ignore", over="ignore"):
                    c = np.where(b[run], -Lam[run], Lam[run])
                    delta = w * c + delta
            assert delta.dtype == np.float32
            b[run] ^= delta < th
            s[run] = syndrome(b[run])
        ok = ~s[act].any(axis=1)
        conv[act[ok]] = it
        act = act[~ok]
        if len(act) == 0:
            break
    iters = np.where(conv >= 0, conv + 1, int(T)).astype(np.int32)
    return dict(z=(~b).astype(np.uint8), conv=conv, status=(conv < 0).astype(np.int32), iters=iters,
                synw=s.sum(axis=1).astype(np.int32))
