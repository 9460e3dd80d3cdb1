"""numpy int32 restatement of physical mode's fixed-point min-sum decoder
(DESIGN.md "Physical mode: fixed-point min-sum"; include/ldpc_hip.h
ldpc_phys_decode_q).  A helper module, not a test.

All integer arithmetic is exact, so the GPU decoder must reproduce every output:
  Qmax = 2^(q-1) - 1,  Pmax = 2^(q+1) - 1
  load (fp32, each operation rounds once):  x = (-(float)llr) * llr_scale
      Lam = (int)clamp(rint(x), -Qmax, Qmax)   rint: half to even; L = Lam, E = 0
  per row, edges in CSR order:  Q = clamp(L[c] - E, -Qmax, Qmax), a = |Q|, s = (Q < 0)
      mag_e = min of a over the other edges  (min2 at the argmin, else min1)
      nms: mag = (alpha_q * mag + 8) >> 4      oms: mag = max(mag - beta_q, 0)
      R_e = -mag if parity(all s) ^ s_e else mag
  flooding: all rows from the same L and E, E = R, then
            L[j] = clamp(Lam[j] + sum of E over column j's edges, -Pmax, Pmax)
  layered:  layer after layer, L[c_e] = Q_e + R_e, E_e = R_e  (no clamp: |L| <= 2 Qmax)
  after each full iteration b = (L < 0); conv = first iteration with H b = 0.
Frames are vectorised; a frame that has converged is left alone.  Besides the
outputs, decode() counts what the quantizer did (over the frames while they
run): Lam values at +-Qmax, Q clamps that bit, posterior clamps that bit and
posteriors equal to 0.
"""
import numpy as np
from scipy import sparse

from minsum_ref import _Code


def limits(qbits):
    """(Qmax, Pmax)."""
    return (1 << (qbits - 1)) - 1, (1 << (qbits + 1)) - 1


def quantize(llr, qbits, llr_scale):
    """Lam int32 of fp64 channel LLRs (the contract's load)."""
    qmax = np.float32(limits(qbits)[0])
    x = (-(np.asarray(llr, dtype=np.float64).astype(np.float32))) * np.float32(llr_scale)
    assert x.dtype == np.float32
    return np.clip(np.rint(x), -qmax, qmax).astype(np.int32)


def check(Q, cn, param_q):
    """R [..., d] int32 from the clamped Q [..., d] int32."""
    a = np.abs(Q)
    arg = a.argmin(axis=-1)
    min1 = np.take_along_axis(a, arg[..., None], -1)
    rest = a.copy()
    np.put_along_axis(rest, arg[..., None], np.int32(1 << 20), -1)
    min2 = rest.min(axis=-1, keepdims=True)
    mag = np.where(np.arange(a.shape[-1]) == arg[..., None], min2, min1)
    if cn == "nms":
        mag = (np.int32(param_q) * mag + 8) >> 4
    else:
        mag = np.maximum(mag - np.int32(param_q), 0)
    s = Q < 0
    flip = (s.sum(axis=-1, keepdims=True) & 1).astype(bool) ^ s
    return np.where(flip, -mag, mag).astype(np.int32)


_CODES = {}


def decode(H, llr, max_iter, cn="nms", schedule="flooding", qbits=6, llr_scale=4.0, param_q=12):
    """dict(z, conv, status, iters, post int16, counts) as
    ldpc_amd.device.phys_decode(..., qbits=) returns them; counts = dict(lam_sat,
    q_clamps, post_clamps, post_zero)."""
    assert cn in ("nms", "oms") and schedule in ("flooding", "layered") and 4 <= qbits <= 8
    qmax, pmax = limits(qbits)
    assert 1 <= param_q <= 16 if cn == "nms" else 0 <= param_q <= qmax
    H = sparse.csr_matrix(H)
    key = (H.shape, H.indptr.tobytes(), H.indices.tobytes())
    code = _CODES.get(key) or _CODES.setdefault(key, _Code(H))
    Lam_all = quantize(np.atleast_2d(llr), qbits, llr_scale)
    B = Lam_all.shape[0]
    counts = dict(lam_sat=int((np.abs(Lam_all) == qmax).sum()), q_clamps=0, post_clamps=0, post_zero=0)
    post = Lam_all.copy()
    conv = np.full(B, -1, np.int32)
    act = np.arange(B)  # frames still running; their state:
    Lam, L, E = Lam_all.copy(), Lam_all.copy(), np.zeros((B, len(code.cols)), np.int32)

    def clampq(D):
        counts["q_clamps"] += int((np.abs(D) > qmax).sum())
        return np.clip(D, -qmax, qmax)

    for it in range(int(max_iter)):
        if schedule == "flooding":
            R = np.empty_like(E)
            for e, c in code.all_rows:
                R[:, e] = check(clampq(L[:, c] - E[:, e]), cn, param_q)
            E = R
            S = Lam.copy()
            for j, e in code.vn_steps:
                S[:, j] += E[:, e]
            counts["post_clamps"] += int((np.abs(S) > pmax).sum())
            L = np.clip(S, -pmax, pmax)
        else:
            for layer in code.layers:
                for e, c in layer:
                    Q = clampq(L[:, c] - E[:, e])
                    R = check(Q, cn, param_q)
                    L[:, c] = Q + R
                    E[:, e] = R
            assert np.abs(L).max(initial=0) <= 2 * qmax < pmax  # no posterior clamp in this schedule
        assert L.dtype == np.int32 and E.dtype == np.int32
        counts["post_zero"] += int((L == 0).sum())
        post[act] = L
        ok = code.syndrome_ok(L)
        conv[act[ok]] = it
        act, Lam, L, E = act[~ok], Lam[~ok], L[~ok], E[~ok]
        if len(act) == 0:
            break
    iters = np.where(conv >= 0, conv + 1, int(max_iter)).astype(np.int32)
    assert np.abs(post).max(initial=0) <= pmax
    return dict(z=(post >= 0).astype(np.uint8), conv=conv, status=(conv < 0).astype(np.int32), iters=iters,
                post=post.astype(np.int16), counts=counts)
