"""The reference database's other code shapes (DESIGN.md "Parity decoder on
the database's other shapes"): ten matrices that sit on the limits the kernel
choice branches on, beside the five codes the package ships.

tests/golden/db/codes/<name>.npz  the reference's own record of a code: H as
    CSR, m_std, k, the column permutation and sha256 pins of H_std (full H_std
    where the file stays small) -- same fields as ldpc_amd/codes/*.npz;
tests/golden/db/<set>.npz         4 frames at T = 3 decoded by the reference
    itself, both Result values among them (tests/golden/gen_golden.py DB_SETS).

Kept out of tests/golden/*.npz and of the package's codes/ on purpose: the
parametrized tests over the five shipped codes glob those directories.
"""
import glob
import os

import numpy as np
from scipy import sparse

DB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "db")

# golden set -> code
SETS = {
    "ccsds32_T3": "CCSDS_ldpc_n32_k16",
    "tanner155_T3": "Tanner_155_64",
    "wran480_T3": "WRAN_N480_K240_R05",
    "wran384_T3": "WRAN_N384_K320_R083",
    "wigig672_T3": "wigig_R05_N672_K336",
    "ad672_T3": "ieee_802_11ad_n672_r081",
    "w1152_83_T3": "wimax_1152_0.83",
    "w1440_T3": "wimax_1440_0.5",
    "w2304_66B_T3": "wimax_2304_0.66B",
    "w2304_83_T3": "wimax_2304_0.83",
}
CODES = list(SETS.values())
SET_OF = {c: s for s, c in SETS.items()}

# What each code is here for, as pinned by the reference's standard form:
# (k, m_std, min row degree, max row degree, max column degree, 2*odd_rows <= m).
# tests/test_db_codes_host.py holds the fixtures to this table, so one
# regenerated differently cannot quietly stop covering its limit.
SHAPES = {
    "CCSDS_ldpc_n32_k16": (16, 16, 6, 12, 9, True),          # k half a word, m < 32
    "Tanner_155_64": (64, 91, 26, 49, 61, True),             # rank-deficient (93 rows -> 91); k exactly 2 words
    "WRAN_N480_K240_R05": (240, 240, 60, 140, 142, False),   # 140 odd rows of 240: lpt_weak_id = 0
    "WRAN_N384_K320_R083": (320, 64, 148, 256, 43, True),    # k = 320 (tile_kernel's limit), rows > 192
    "wigig_R05_N672_K336": (336, 336, 42, 193, 192, True),   # one edge over cn_row / tile_kernel's 192
    "ieee_802_11ad_n672_r081": (546, 126, 42, 301, 83, True),  # k = 17 words + 2 bits
    "wimax_1152_0.83": (960, 192, 20, 520, 127, True),       # very uneven rows
    "wimax_1440_0.5": (720, 720, 300, 480, 407, True),       # mid-size: sub16 and tile8 both fit
    "wimax_2304_0.66B": (1536, 768, 96, 644, 429, True),     # 4 edges over sub16's / cn_row16's 640; cn_sub shape 30
    "wimax_2304_0.83": (1920, 384, 864, 1030, 226, True),    # over the edge path's 1024 and cn_sub's 960
}


def load_db_code(name):
    return np.load(os.path.join(DB, "codes", f"{name}.npz"), allow_pickle=False)


def db_H(name):
    """The matrix as the reference read it from its database (before the standard form)."""
    c = load_db_code(name)
    return sparse.csr_matrix((c["h_data"], c["h_indices"], c["h_indptr"]), shape=(int(c["m"]), int(c["n"])))


_HSTD = {}


def db_hstd(name):
    """H_std by the native builder, checked against the reference's sha256 pin."""
    if name not in _HSTD:
        import ldpc_amd
        Hs, _ = ldpc_amd.build_standard_form(db_H(name))
        assert ldpc_amd.csr_fingerprint(Hs) == str(load_db_code(name)["hstd_sha"]), name
        _HSTD[name] = Hs
    return _HSTD[name]


def load_db_golden(set_name):
    """As conftest.load_golden, from tests/golden/db/ (one file or consecutive parts)."""
    whole = os.path.join(DB, f"{set_name}.npz")
    if os.path.exists(whole):
        g = np.load(whole, allow_pickle=False)
        return {k: g[k] for k in g.files}
    paths = glob.glob(os.path.join(DB, f"{set_name}.part*.npz"))
    parts = [np.load(p, allow_pickle=False) for p in sorted(paths, key=lambda p: int(p[:-4].rsplit(".part", 1)[1]))]
    assert parts, f"no golden set {set_name}"
    return {k: parts[0][k] if parts[0][k].ndim == 0 else np.concatenate([p[k] for p in parts]) for k in parts[0].files}
