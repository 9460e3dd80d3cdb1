"""numpy float64 statement of physical mode's sum-product decoder (the
contract of ldpc_phys_decode, include/ldpc_hip.h; csrc/phys_kernels.hip).  A
helper module, not a test.

  Lam = -(float32)llr, widened to float64;  L = Lam, E = 0
  phi(x) = -log tanh(x / 2), x clamped to [float32(1e-7), 30]
  per row, edges in CSR order:  M = L[c] - E,  S = sum phi(|M|)
      mag_e = phi(max(S - phi(|M_e|), 0)),  E_e = -mag_e iff the other edges'
      (M < 0) have odd parity, else mag_e
  flooding:  L[j] = Lam[j] + sum of E over column j's edges
No early exit: decode() returns the posterior after exactly T iterations, and
beside it what the exit rule would have done (conv: the first iteration whose
b = (L < 0) has H b = 0) and how far each frame's posteriors stayed from 0 on
the columns that have edges, so a test can tell a decided frame from a marginal one.
"""
import numpy as np
from scipy import sparse

from minsum_ref import _Code

PHI_MIN = float(np.float32(1e-7))
PHI_MAX = 30.0


def phi(x):
    """log((1 + e^-x) / (1 - e^-x)) = -log tanh(x / 2) on the clamped x."""
    x = np.clip(np.asarray(x, dtype=np.float64), PHI_MIN, PHI_MAX)
    t = np.exp(-x)
    # 1 - e^-x without cancellation at either end of the range
    return np.log1p(t) - np.where(x < 1.0, np.log(-np.expm1(-x)), np.log1p(-t))


_CODES = {}


def decode(H, llr, T):
    """dict(post float64 [B, n] after exactly T iterations, conv int32 [B],
    margin float64 [B]: min over the iterations and the columns with edges of |L|)."""
    H = sparse.csr_matrix(H)
    key = (H.shape, H.indptr.tobytes(), H.indices.tobytes())
    code = _CODES.get(key) or _CODES.setdefault(key, _Code(H))
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    B = llr.shape[0]
    Lam = (-(llr.astype(np.float32))).astype(np.float64)
    L, E = Lam.copy(), np.zeros((B, len(code.cols)), np.float64)
    conv = np.full(B, -1, np.int32)
    margin = np.full(B, np.inf)
    has_edge = np.bincount(code.cols, minlength=code.n) > 0
    for it in range(int(T)):
        R = np.empty_like(E)
        for e, c in code.all_rows:
            M = L[:, c] - E[:, e]
            p = phi(np.abs(M))
            S = p.sum(axis=-1, keepdims=True)
            mag = phi(np.maximum(S - p, 0.0))
            s = M < 0
            flip = (s.sum(axis=-1, keepdims=True) & 1).astype(bool) ^ s
            R[:, e] = np.where(flip, -mag, mag)
        E = R
        L = Lam.copy()
        for j, e in code.vn_steps:
            L[:, j] = L[:, j] + E[:, e]
        margin = np.minimum(margin, np.abs(L[:, has_edge]).min(axis=1))
        ok = code.syndrome_ok(L)
        conv[(conv < 0) & ok] = it
    return dict(post=L, conv=conv, margin=margin)
