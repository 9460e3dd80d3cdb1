"""numpy fp32 restatement of physical mode's min-sum rules and schedules
(DESIGN.md "Physical mode: min-sum rules and the layered schedule";
include/ldpc_hip.h LDPC_CN_*, LDPC_SCHED_*).  A helper module, not a test.

Every step is one fp32 operation on fp32 arrays, in the order the contract
fixes, so the GPU decoders (built without FMA contraction) must reproduce it
bit for bit:
  Lam = -(float)llr, L = Lam, E = 0
  per row, edges in CSR order:  Q = L[c] - E,  a = |Q|,  s = (Q < 0)
      mag_e = min of a over the other edges  (min2 at the argmin, else min1)
      nms: mag = alpha * mag        oms: mag = max(mag - beta, 0)
      R_e = -mag if parity(all s) ^ s_e else mag
  flooding: all rows from the same L and E, E = R, then
            L[j] = Lam[j] + E_0 + E_1 + ... over column j's edges, rows ascending
  layered:  layer after layer, L[c_e] = Q_e + R_e, E_e = R_e
  after each full iteration b = (L < 0); conv = first iteration with H b = 0.
Frames are vectorised; a frame that has converged is left alone.
"""
import numpy as np
from scipy import sparse


def first_fit_layers(H):
    """(layer_ptr, layer_rows) int32: rows in ascending order, each into the
    lowest-numbered layer none of whose rows shares a column with it."""
    H = sparse.csr_matrix(H)
    used = []  # per layer: bool [n]
    of_row = np.empty(H.shape[0], np.int64)
    for r in range(H.shape[0]):
        cols = H.indices[H.indptr[r]:H.indptr[r + 1]]
        for l, u in enumerate(used):
            if not u[cols].any():
                break
        else:
            used.append(np.zeros(H.shape[1], bool))
            l = len(used) - 1
        used[l][cols] = True
        of_row[r] = l
    layer_ptr = np.zeros(len(used) + 1, np.int32)
    np.cumsum(np.bincount(of_row, minlength=len(used)), out=layer_ptr[1:])
    return layer_ptr, np.argsort(of_row, kind="stable").astype(np.int32)


class _Code:
    """Index tables of one graph (rows grouped by degree so a group is a dense block)."""

    def __init__(self, H):
        H = sparse.csr_matrix(H)
        H.sort_indices()
        self.m, self.n = H.shape
        self.indptr = H.indptr.astype(np.int64)
        self.cols = H.indices.astype(np.int64)
        self.deg = np.diff(self.indptr)
        if self.deg.min() < 2:
            raise ValueError("min-sum needs every row to have at least 2 edges")
        # CSC view, rows ascending within a column: position k of every column that has one
        order = np.argsort(self.cols, kind="stable")  # edges by column, CSR (row) order kept
        cptr = np.zeros(self.n + 1, np.int64)
        np.cumsum(np.bincount(self.cols, minlength=self.n), out=cptr[1:])
        cdeg = np.diff(cptr)
        self.vn_steps = []
        for k in range(int(cdeg.max())):
            j = np.nonzero(cdeg > k)[0]
            self.vn_steps.append((j, order[cptr[j] + k]))
        self.all_rows = self.groups(np.arange(self.m))
        lp, lr = first_fit_layers(H)
        self.layers = [self.groups(lr[lp[l]:lp[l + 1]].astype(np.int64)) for l in range(len(lp) - 1)]

    def groups(self, rows):
        """[(edge ids [rows_d, d], their columns)] for each degree d among `rows`."""
        out = []
        for d in np.unique(self.deg[rows]):
            r = rows[self.deg[rows] == d]
            e = self.indptr[r][:, None] + np.arange(d)[None, :]
            out.append((e, self.cols[e]))
        return out

    def syndrome_ok(self, L):
        b = (L[:, self.cols] < 0).astype(np.int32)
        return ((np.add.reduceat(b, self.indptr[:-1], axis=1) & 1) == 0).all(axis=1)


def _check(Q, cn, param):
    """R [B, rows, d] from Q [B, rows, d]."""
    a = np.abs(Q)
    arg = a.argmin(axis=-1)
    min1 = np.take_along_axis(a, arg[..., None], -1)
    rest = a.copy()
    np.put_along_axis(rest, arg[..., None], np.float32(np.inf), -1)
    min2 = rest.min(axis=-1, keepdims=True)
    mag = np.where(np.arange(a.shape[-1]) == arg[..., None], min2, min1)
    if cn == "nms":
        mag = np.float32(param) * mag
    else:
        mag = np.maximum(mag - np.float32(param), np.float32(0.0))
    assert mag.dtype == np.float32
    s = Q < 0
    flip = (s.sum(axis=-1, keepdims=True) & 1).astype(bool) ^ s
    return np.where(flip, -mag, mag)


_CODES = {}


def decode(H, llr, max_iter, cn="nms", schedule="flooding", alpha=0.75, beta=0.5):
    """dict(z, conv, status, iters, post) as ldpc_amd.device.phys_decode returns them."""
    assert cn in ("nms", "oms") and schedule in ("flooding", "layered")
    H = sparse.csr_matrix(H)
    key = (H.shape, H.indptr.tobytes(), H.indices.tobytes())
    code = _CODES.get(key) or _CODES.setdefault(key, _Code(H))
    param = alpha if cn == "nms" else beta
    llr = np.atleast_2d(np.asarray(llr, dtype=np.float64))
    B = llr.shape[0]
    Lam_all = -(llr.astype(np.float32))
    post = Lam_all.copy()
    conv = np.full(B, -1, np.int32)
    act = np.arange(B)  # frames still running; their state:
    Lam, L, E = Lam_all.copy(), Lam_all.copy(), np.zeros((B, len(code.cols)), np.float32)
    for it in range(int(max_iter)):
        if schedule == "flooding":
            R = np.empty_like(E)
            for e, c in code.all_rows:
                R[:, e] = _check(L[:, c] - E[:, e], cn, param)
            E = R
            L = Lam.copy()
            for j, e in code.vn_steps:
                L[:, j] = L[:, j] + E[:, e]
        else:
            for layer in code.layers:
                for e, c in layer:
                    Q = L[:, c] - E[:, e]
                    R = _check(Q, cn, param)
                    L[:, c] = Q + R
                    E[:, e] = R
        assert L.dtype == np.float32 and E.dtype == np.float32
        post[act] = L
        ok = code.syndrome_ok(L)
        conv[act[ok]] = it
        act, Lam, L, E = act[~ok], Lam[~ok], L[~ok], E[~ok]
        if len(act) == 0:
            break
    iters = np.where(conv >= 0, conv + 1, int(max_iter)).astype(np.int32)
    return dict(z=(post >= 0).astype(np.uint8), conv=conv, status=(conv < 0).astype(np.int32), iters=iters, post=post)
