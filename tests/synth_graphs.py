"""Small irregular graphs for physical mode's kernel variants, generated in
code from a seed (no fixture files).  A helper module, not a test.

The committed codes are quasi-cyclic with m and n multiples of 32, row degrees
4-7 / 14-15 and column degrees <= 6: they reach one register shape per code and
none of the ragged-edge guards.  Each graph here is built to reach a kernel
variant or a branch the committed codes do not (tests/test_synth_graphs.py
asserts the structure from the matrix; tests/test_gpu_phys_shapes.py runs them):

  name       m     n     structure                               reaches
  ragged     37    101   rows of 2,3,5,7,8; columns of 0,1,8     reg {1,8,1,8}; HBM cn<8>/vn<8>, ragged m and n
  shape2     700   1400  rows of 5-8; columns <= 6 (one of 6)    reg {2,8,3,8}; phys_quant_reg_kernel
  deg16      520   2100  rows of 9,11,15,16                      reg {2,16,5,8}; HBM cn<16>; generic quant
  widecol    61    121   a column of 12, one of 9                generic phys_kernel; HBM vn<0>; generic quant
  longrow    200   1203  rows of 17,24,32,33,40                  generic phys_kernel; HBM cn<32> + long rows
  large      1300  2602  rows of 6-7                             no reg shape (6 columns per thread)
  widelayer  1200  2400  QC, z=300, 4x8 base with zero blocks    a layer of > 256 rows
  pairs      256   512   row r = columns 2r, 2r+1                phi sweep

Every graph is a scipy CSR with sorted rows, m <= n, every row >= 2 edges.
A row is dealt its degree from the least-used columns (ties by the seed); the
named column degrees do not arise by chance and are placed first.
"""
import functools

import numpy as np
from scipy import sparse

SEED = 20260307
NAMES = ("ragged", "shape2", "deg16", "widecol", "longrow", "large", "widelayer", "pairs")
# noise per graph at which, of 70 all-zero-codeword frames and 10 iterations,
# some frames reach H b = 0 and some do not in every restatement the tests use
# (asserted there)
SIGMA = {"ragged": 0.8, "shape2": 0.8, "deg16": 0.6, "widecol": 0.8, "longrow": 0.5, "large": 0.82,
         "widelayer": 0.7}
FRAMES = 70  # one full 64-frame HBM tile and a ragged one
# the kernels the flooding decoders run each graph with: (fp32, fixed point)
KERNELS = {"ragged": ("phys_reg_kernel", "phys_quant_kernel"), "shape2": ("phys_reg_kernel", "phys_quant_reg_kernel"),
           "deg16": ("phys_reg_kernel", "phys_quant_kernel"), "widecol": ("phys_kernel", "phys_quant_kernel"),
           "longrow": ("phys_kernel", "phys_quant_kernel"), "large": ("phys_kernel", "phys_quant_kernel"),
           "widelayer": ("phys_reg_kernel", "phys_quant_reg_kernel"),
           "pairs": ("phys_reg_kernel", "phys_quant_reg_kernel")}


def _csr(m, n, rows):
    indptr = np.zeros(m + 1, np.int32)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = np.concatenate([np.sort(np.fromiter(r, np.int64, len(r))) for r in rows]).astype(np.int32)
    H = sparse.csr_matrix((np.ones(len(indices), np.int8), indices, indptr), shape=(m, n))
    H.has_sorted_indices = True
    return H


def _deal(m, n, degs, seed, placed=None, empty=()):
    """Rows of the given degrees.  placed: {column: rows that hold it} (fixed
    degrees); empty: columns left without edges; the rest is dealt from the
    least-used columns."""
    rng = np.random.default_rng(seed)
    placed = placed or {}
    rows = [set() for _ in range(m)]
    for c, rr in placed.items():
        assert len(set(rr)) == len(rr)
        for r in rr:
            rows[r].add(c)
    free = np.ones(n, bool)
    free[list(empty) + list(placed)] = False
    use = np.zeros(n, np.float64)
    for r in range(m):
        need = degs[r] - len(rows[r])
        assert need >= 0
        key = use + rng.random(n)
        key[~free] = np.inf
        pick = np.argsort(key)[:need]
        assert np.isfinite(key[pick]).all()
        rows[r].update(int(c) for c in pick)
        use[pick] += 1
    return _csr(m, n, rows)


def _cycle(m, degs):
    return [degs[r % len(degs)] for r in range(m)]


def _rows_with(degs, seed, count, at_least):
    """`count` distinct rows of degree >= at_least, chosen by the seed."""
    ok = np.nonzero(np.asarray(degs) >= at_least)[0]
    return sorted(int(r) for r in np.random.default_rng(seed).choice(ok, size=count, replace=False))


def _ragged():
    m, n = 37, 101
    degs = _cycle(m, (2, 3, 5, 7, 8))
    # column 7 in exactly 8 rows; columns 37 and 100 (the last, in the ragged column block) empty
    return _deal(m, n, degs, SEED + 1, placed={7: _rows_with(degs, SEED + 11, 8, 3)}, empty=(37, 100))


def _shape2():
    m, n = 700, 1400
    degs = _cycle(m, (5, 6, 7, 8))
    return _deal(m, n, degs, SEED + 2, placed={n - 1: _rows_with(degs, SEED + 12, 6, 5)})


def _deg16():
    m, n = 520, 2100
    return _deal(m, n, _cycle(m, (9, 11, 15, 16)), SEED + 3)


def _widecol():
    m, n = 61, 121
    degs = _cycle(m, (3, 4, 5, 6))
    # the column of 12 is the last one (the ragged column block), the column of 9 sits in a full block
    return _deal(m, n, degs, SEED + 4, placed={n - 1: _rows_with(degs, SEED + 13, 12, 4),
                                               8: _rows_with(degs, SEED + 14, 9, 5)})


def _longrow():
    m, n = 200, 1203
    return _deal(m, n, _cycle(m, (17, 24, 32, 33, 40)), SEED + 5)


def _large():
    m, n = 1300, 2602
    return _deal(m, n, _cycle(m, (6, 7)), SEED + 6)


def _widelayer():
    """Quasi-cyclic, z = 300: block row i of the base matrix is 300 rows that
    share no column, so first-fit puts at least 300 rows into one layer."""
    z = 300
    base = np.array([[1, 1, 0, 1, 1, 0, 1, 0],
                     [0, 1, 1, 0, 1, 1, 0, 1],
                     [1, 0, 1, 1, 0, 1, 1, 0],
                     [1, 1, 1, 0, 0, 0, 1, 1]])
    rng = np.random.default_rng(SEED + 7)
    shift = rng.integers(0, z, size=base.shape)
    rows = []
    for i in range(base.shape[0]):
        for t in range(z):
            rows.append({j * z + (t + int(shift[i, j])) % z for j in range(base.shape[1]) if base[i, j]})
    return _csr(base.shape[0] * z, base.shape[1] * z, rows)


def _pairs():
    return _csr(256, 512, [{2 * r, 2 * r + 1} for r in range(256)])


_BUILD = {"ragged": _ragged, "shape2": _shape2, "deg16": _deg16, "widecol": _widecol, "longrow": _longrow,
          "large": _large, "widelayer": _widelayer, "pairs": _pairs}


@functools.lru_cache(maxsize=None)
def graph(name):
    """The graph, built once and shared (read-only)."""
    H = _BUILD[name]()
    for a in (H.data, H.indices, H.indptr):
        a.setflags(write=False)
    return H


def degrees(H):
    """(row degrees [m], column degrees [n])."""
    return np.diff(H.indptr), np.bincount(H.indices, minlength=H.shape[1])


# ---- frames
def noisy_frames(n, sigma, count, seed):
    """All-zero codeword, BPSK bit 0 -> -1, y = -1 + sigma N(0, 1), llr = 2 y / sigma^2."""
    y = -1.0 + sigma * np.random.default_rng(seed).standard_normal((count, n))
    return 2.0 * y / sigma ** 2


# the hand-made frame's values, each group on columns of one row: signed zeros;
# two equal magnitudes of opposite sign that are the row's smallest (min1 =
# min2: the row's other values are raised to magnitude 1 at least); the fp32
# range's ends, a value that is denormal after the fp32 load, and the
# quantizer's ties at scale 4
HAND_GROUPS = ((0.0, -0.0), (0.25, -0.25), (1e30, -1e30, 1e-40, 0.625, 0.875))
HAND_TIE = 1  # the group that must stay the smallest of its row


def hand_frame(H, base):
    """`base` (one frame) with HAND_GROUPS written over columns that share rows:
    group g onto the first len(g) columns of the first row all of whose columns
    no earlier group took."""
    out = np.array(base, dtype=np.float64)
    taken = np.zeros(H.shape[1], bool)
    for g, grp in enumerate(HAND_GROUPS):
        for r in range(H.shape[0]):
            cols = H.indices[H.indptr[r]:H.indptr[r + 1]]
            if len(cols) >= len(grp) and not taken[cols].any():
                if g == HAND_TIE:
                    out[cols] = np.copysign(np.maximum(np.abs(out[cols]), 1.0), out[cols])
                out[cols[:len(grp)]] = grp
                taken[cols] = True
                break
        else:
            raise AssertionError("no row takes the group")
    return out


@functools.lru_cache(maxsize=None)
def frames(name, count=FRAMES, hand=True):
    """`count` noisy frames at SIGMA[name] and, with `hand`, the hand-made frame
    appended as the last one.  Shared, read-only."""
    H = graph(name)
    llr = noisy_frames(H.shape[1], SIGMA[name], count + (1 if hand else 0), SEED + 100 + NAMES.index(name))
    if hand:
        llr[-1] = hand_frame(H, llr[-1])
    llr.setflags(write=False)
    return llr


# ---- the exact rules' restatements on those frames, computed once per case
ALPHA, BETA = 0.75, 0.5
QBITS, QSCALE, ALPHA_Q, BETA_Q = 6, 4.0, 12, 2
# the rule of each graph's layered case (half the graphs each)
LAYERED_RULE = {"ragged": "nms", "shape2": "oms", "deg16": "nms", "widecol": "oms", "longrow": "nms",
                "large": "oms", "widelayer": "nms"}
# the fixed-point cases of each graph: (rule, schedule, param_q)
Q_CASES = (("nms", "flooding", ALPHA_Q), ("nms", "layered", ALPHA_Q))
Q_OMS_GRAPH = "shape2"  # plus ("oms", "flooding", BETA_Q) on this one


def _frozen(r):
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def ms_ref(name, cn, schedule, T=10, count=FRAMES, hand=True):
    import minsum_ref
    return _frozen(minsum_ref.decode(graph(name), frames(name, count, hand), T, cn, schedule, ALPHA, BETA))


@functools.lru_cache(maxsize=None)
def q_ref(name, cn, schedule, param_q, T=10):
    import qminsum_ref
    return _frozen(qminsum_ref.decode(graph(name), frames(name), T, cn, schedule, QBITS, QSCALE, param_q))


def exact_cases(name):
    """Every restatement the GPU tests compare graph `name` with, as (label, result)."""
    out = [("nms flooding", ms_ref(name, "nms", "flooding")), ("oms flooding", ms_ref(name, "oms", "flooding")),
           (f"{LAYERED_RULE[name]} layered", ms_ref(name, LAYERED_RULE[name], "layered"))]
    out += [(f"q {cn} {sch}", q_ref(name, cn, sch, pq)) for cn, sch, pq in Q_CASES]
    if name == Q_OMS_GRAPH:
        out.append(("q oms flooding", q_ref(name, "oms", "flooding", BETA_Q)))
    return out


def both_exits(r):
    """Of the noisy frames at least 3 reach H b = 0 and at least 3 do not."""
    ok = int((r["status"][:FRAMES] == 0).sum())
    return 3 <= ok <= FRAMES - 3


# ---- sum-product inputs (tests against spa_ref64)
SPA_SHORT = {1: 6.0, 2: 3.0}  # iterations -> the llr are uniform in [-a, a]


@functools.lru_cache(maxsize=None)
def spa_short_frames(name, T):
    """8 frames of uniform llr for a T-iteration comparison with float64.  Shared, read-only."""
    a = SPA_SHORT[T]
    llr = np.random.default_rng(SEED + 200 + 10 * NAMES.index(name) + T).uniform(-a, a, (8, graph(name).shape[1]))
    llr.setflags(write=False)
    return llr


PHI_OWN = (0.5, 4.0, 12.0)  # the even columns' Lambda, one value per frame
_B = np.float32(0.03125)    # phi's branch point
# |x| below 8: the clamp at 1e-7 from both sides, the series branch, the branch
# point itself with its fp32 neighbours and near neighbours, a geometric grid
PHI_SMALL = np.concatenate([
    [0.0, 1e-9, 1e-7, 5e-5],
    [float(np.nextafter(_B, np.float32(0))), float(_B), float(np.nextafter(_B, np.float32(1))), 0.03124, 0.03126],
    np.geomspace(1e-3, 7.9, 60)])
# |x| from 8: fp32 phi is quantised by design; past the clamp at 30; the fp32 range's end
# (none equal to an own value: x = -own leaves both posteriors of the row at 0)
PHI_BIG = np.array([8.0, 9.0, 10.0, 11.0, 13.0, 14.0, 16.0, 17.0, 20.0, 25.0, 30.0, 31.0, 40.0, 60.0, 1e30])


@functools.lru_cache(maxsize=None)
def phi_sweep():
    """(llr [3, 512], x [256]) on `pairs`: frame i holds Lambda = PHI_OWN[i] on
    every even column; odd column 2r+1 holds Lambda = x[r]: PHI_SMALL then
    PHI_BIG, positive on rows 0..K-1, negated on rows K..2K-1 (so +0.0 and
    -0.0 both occur), 1.0 on the rows left.  llr = -Lambda."""
    mag = np.concatenate([PHI_SMALL, PHI_BIG])
    K = len(mag)
    assert 2 * K <= 256
    x = np.ones(256)
    x[:K], x[K:2 * K] = mag, -mag
    llr = np.empty((len(PHI_OWN), 512))
    for i, own in enumerate(PHI_OWN):
        llr[i, 0::2] = -own
        llr[i, 1::2] = -x
    llr.setflags(write=False)
    x.setflags(write=False)
    return llr, x


# ---- sum-product cases: the float64 contract, the fp32 libm restatement and
# the bound the GPU must keep, 8 x max |restatement - float64| over the same case
SPA_GRAPHS = ("ragged", "shape2", "deg16", "longrow")
SPA_FACTOR = 8.0


@functools.lru_cache(maxsize=None)
def spa_case(name, T):
    import oracle
    import spa_ref64
    H, llr = graph(name), spa_short_frames(name, T)
    ref, orc = spa_ref64.decode(H, llr, T), oracle.phys_decode(H, llr, T)
    err = float(np.abs(orc["post"].astype(np.float64) - ref["post"]).max())
    return _frozen(dict(llr=llr, ref=_frozen(ref), oracle=_frozen(orc), err=err, bound=SPA_FACTOR * err))


@functools.lru_cache(maxsize=None)
def phi_case():
    """The sweep on `pairs`, one iteration.  tight [3, 512]: the values the
    bound applies to -- those that received a message made from a Lambda below
    8 in magnitude: the even columns of the rows with |x| < 8 and, in the frames
    whose own value is below 8, the odd columns.  The rest received
    phi(S - phi(.)) of a phi below 7e-4, which fp32 quantises by design."""
    import oracle
    import spa_ref64
    H = graph("pairs")
    llr, x = phi_sweep()
    ref, orc = spa_ref64.decode(H, llr, 1), oracle.phys_decode(H, llr, 1)
    tight = np.zeros(llr.shape, bool)
    tight[:, 0::2] = np.abs(x) < 8.0
    tight[:, 1::2] = (np.asarray(PHI_OWN) < 8.0)[:, None]
    d = np.abs(orc["post"].astype(np.float64) - ref["post"])
    err = float(d[tight].max())
    return _frozen(dict(llr=llr, x=x, tight=tight, ref=_frozen(ref), oracle=_frozen(orc), err=err,
                        err_loose=float(d[~tight].max()), bound=SPA_FACTOR * err))
