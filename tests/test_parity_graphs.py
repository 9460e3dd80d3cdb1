"""The synthetic limit graphs of tests/parity_graphs.py are what their table
says (CPU): [A | I_m] in canonical CSR, the limiting degree on exactly one row
or column with every other one far shorter, every A column used unless named
empty, and frames on which the oracle takes both exits."""
import numpy as np
import pytest

import parity_graphs as pg


@pytest.mark.parametrize("name", pg.NAMES)
def test_structure(name):
    H = pg.graph(name)
    m, k, long_deg, long_row = pg.SPEC[name]
    assert H.shape == (m, k + m) and H.has_canonical_format
    np.testing.assert_array_equal(H[:, k:].toarray(), np.eye(m, dtype=H.dtype))
    for r in range(m):
        cols = H.indices[H.indptr[r]:H.indptr[r + 1]]
        assert (np.diff(cols) > 0).all() and cols[-1] == k + r
    deg = np.diff(H.indptr)
    used = np.bincount(H[:, :k].indices, minlength=k)
    empty = pg.EMPTY_COLS if name == "emptycol" else ()
    assert sorted(np.nonzero(used == 0)[0]) == sorted(empty)
    if long_deg is not None:
        assert deg[long_row] == long_deg == deg.max()
        assert np.delete(deg, long_row).max() <= max(pg.SHORT)
    if name.startswith("k"):
        assert deg.max() <= 57 and k == int(name[1:])
    if name.startswith("c"):
        assert used[pg.DENSE_COL] == int(name[1:]) == used.max()
        assert np.delete(used, pg.DENSE_COL).max() < 200 and deg.max() <= 4
    if name == "idrow":
        assert deg[pg.ID_ROW] == 1 and (np.delete(deg, pg.ID_ROW) >= 3).all()


def test_ragged_sizes():
    ms = {pg.SPEC[n][0] for n in pg.NAMES}
    assert sum(1 for m in ms if m % 4 and m < 64) >= 2
    assert all(24 <= pg.SPEC[n][0] <= 48 for n in pg.NAMES if not n.startswith("c"))


def test_pairs_straddle_their_limits():
    rows = {n: pg.shape(n)[3] for n in pg.NAMES}
    for at, over, lim in (("r192k288", "r193k288", 192), ("r192", "r193", 192), ("r640", "r641", 640),
                          ("r960", "r961", 960), ("r1024", "r1025", 1024)):
        assert (rows[at], rows[over]) == (lim, lim + 1)
    assert (pg.shape("k2048")[0], pg.shape("k2049")[0]) == (2048, 2049)
    assert (pg.shape("c1024")[4], pg.shape("c1025")[4]) == (1024, 1025)
    assert (pg.shape("r192")[0], pg.shape("r193")[0]) == (320, 321)


@pytest.mark.parametrize("name", pg.NAMES)
def test_frames_take_both_exits(name):
    llr = pg.frames(name)
    assert llr.shape == (pg.FRAMES, pg.graph(name).shape[1]) and np.isfinite(llr).all()
    r = pg.reference(name)
    assert pg.both_exits(r), (name, int((r["status"] == 0).sum()))
    assert (r["iters"] == pg.T).any()
