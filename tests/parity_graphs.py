"""Small [A | I_m] graphs at the limits of the parity decoder's kernel choice,
generated in code from a seed (no fixture files).  A helper module, not a test.

The database codes of tests/db_codes.py sit near these limits where the
database happens to; each graph here sits exactly ON one (or one edge over):
one row -- or one column -- carries the limiting degree and every other row
is much shorter, so the long-row code and the short-row code run in the same
launch.  m is small and mostly no multiple of 4, 8 or 32 (ragged last word of
the identity bits, ragged row blocks).

  name        m     k     long row   limit
  r192k288    37    288   192        tile_kernel's rows (16 x 12), its LDS still fits
  r193k288    37    288   193          ... one over: the sub-tile decoder instead
  r192        37    320   192        cn_row_kernel's rows (8 x 24); k = 320: tile_kernel's LDS is out
  r193        37    321   193          ... one over: cn_kernel
  r640        41    700   640        sub16 / cn_row16 (16 x 40), cn_sub shape 20 (8 x 4 x 20), tile8 K = 5 + pair
  r641        41    700   641          ... one over: tile8 K = 8, cn_sub shape 30
  r960        43    1000  960        cn_sub shape 30 (8 x 4 x 30)
  r961        43    1000  961          ... one over: cn_kernel
  r1024       45    1100  1024       the edge path (64 x 16) and tile8 K = 8 (16 x 8 x 8)
  r1025       45    1100  1025         ... one over: no edge path, no tile-resident decoder
  k2048       46    2048  ~50        the column-parallel VN's and the edge path's 64 words of (z^1)_A
  k2049       46    2049  ~50          ... one over: neither
  c1024       1042  40    4          the edge path's column limit: column 7 in 1024 rows
  c1025       1042  40    4            ... one over
  emptycol    38    100   13         columns 0 and 50 of A have no edge
  idrow       35    90    13         row 11 has its identity entry only

Degrees count the identity entry.  A's rows are dealt by synth_graphs._deal
(least-used columns first), so every A column is used unless named empty.
"""
import functools

import numpy as np
from scipy import sparse

import synth_graphs as sg

SEED = 20261020
FRAMES, T = 70, 4  # one full 64-frame tile and a ragged one

# name -> (m, k, long-row degree or None, row that carries it)
SPEC = {
    "r192k288": (37, 288, 192, 5), "r193k288": (37, 288, 193, 5),
    "r192": (37, 320, 192, 5), "r193": (37, 321, 193, 5),
    "r640": (41, 700, 640, 40), "r641": (41, 700, 641, 40),
    "r960": (43, 1000, 960, 0), "r961": (43, 1000, 961, 0),
    "r1024": (45, 1100, 1024, 17), "r1025": (45, 1100, 1025, 17),
    "k2048": (46, 2048, None, None), "k2049": (46, 2049, None, None),
    "c1024": (1042, 40, None, None), "c1025": (1042, 40, None, None),
    "emptycol": (38, 100, None, None), "idrow": (35, 90, None, None),
}
NAMES = tuple(SPEC)
SHORT = (3, 5, 8, 13)          # the other rows of the long-row graphs
DENSE_COL = 7                  # c1024 / c1025
EMPTY_COLS = (0, 50)           # emptycol
ID_ROW = 11                    # idrow


def _with_identity(A):
    m = A.shape[0]
    H = sparse.hstack([A, sparse.identity(m, dtype=np.int8, format="csr")], format="csr")
    H.sort_indices()
    return H


@functools.lru_cache(maxsize=None)
def graph(name):
    m, k, long_deg, long_row = SPEC[name]
    seed = SEED + NAMES.index(name)
    placed, empty = None, ()
    if long_deg is not None:
        degs = sg._cycle(m, SHORT)
        degs[long_row] = long_deg
    elif name.startswith("k"):
        degs = sg._cycle(m, (48, 51, 54, 57))           # 46 rows of ~52: every one of k columns used
    elif name.startswith("c"):
        degs = sg._cycle(m, (2, 3, 4))
        col = int(name[1:])                              # column DENSE_COL in exactly that many rows
        rows = np.random.default_rng(seed).choice(m, size=col, replace=False)
        placed = {DENSE_COL: sorted(int(r) for r in rows)}
    elif name == "emptycol":
        degs, empty = sg._cycle(m, SHORT), EMPTY_COLS
    else:
        degs = sg._cycle(m, SHORT)
        degs[ID_ROW] = 1
    return _with_identity(sg._deal(m, k, [d - 1 for d in degs], seed, placed=placed, empty=empty))


# These are weak codes (rate > 0.9, A columns of degree <= 3), so the frames
# are half at one SNR and half at another: at the lower one most frames run
# all T passes and fail, some converge on the way; at the higher one most stop
# at their first pass.  Chosen on the CPU; the tests assert on the oracle's
# output that both exits occur.
SNRS = {
    "r192k288": (10.0, 12.5), "r193k288": (10.0, 12.5), "r192": (10.5, 12.5), "r193": (10.0, 12.5),
    "r640": (9.5, 10.0), "r641": (9.5, 12.0), "r960": (10.0, 12.5), "r961": (9.5, 11.5),
    "r1024": (10.0, 12.5), "r1025": (10.5, 12.5), "k2048": (4.0, 12.0), "k2049": (4.0, 12.0),
    "c1024": (14.0, 14.5), "c1025": (14.0, 14.5), "emptycol": (13.0, 14.5), "idrow": (14.0, 14.5),
}


@functools.lru_cache(maxsize=None)
def frames(name):
    """[FRAMES, n] channel LLRs of random codewords (test_gpu_parity._random_llr's model)."""
    from test_gpu_parity import _random_llr
    H = graph(name)
    lo, hi = SNRS[name]
    seed = 9000 + 2 * NAMES.index(name)
    llr = np.concatenate([_random_llr(H, FRAMES // 2, lo, seed), _random_llr(H, FRAMES - FRAMES // 2, hi, seed + 1)])
    llr.setflags(write=False)
    return llr


@functools.lru_cache(maxsize=None)
def reference(name):
    """oracle.spa_decode of frames(name) at T passes, computed once and shared."""
    import oracle
    return oracle.spa_decode(graph(name), frames(name), T, nllr=True, want_E=True)


def both_exits(r):
    """At least 3 frames reach a zero syndrome and at least 3 do not."""
    ok = int((r["status"] == 0).sum())
    return 3 <= ok <= FRAMES - 3


def shape(name):
    """(k, m, min row degree, max row degree, max column degree)"""
    H = graph(name)
    m, n = H.shape
    deg = np.diff(H.indptr)
    return n - m, m, int(deg.min()), int(deg.max()), int(np.bincount(H.indices, minlength=n).max())
