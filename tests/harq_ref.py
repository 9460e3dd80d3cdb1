"""numpy restatement of the frame source under a HARQ plan (include/ldpc_hip.h,
"HARQ") -- a test helper, not a test.

It shares no code with the kernels.  The bits are ratematch_ref.bits (a plan
changes no bit).  Transmission r is interleave_ref.sent_llr on the bits
c[cols_r] with the Philox key seed_r = (seed + r 0x9E3779B97F4A7C15) mod 2^64;
its LLRs are scattered to the columns cols_r and added, r ascending, to a frame
that starts at +0.0, one fp64 addition each.  The columns no transmission
carries stay +0.0; the shortened ones are -KNOWN_LLR.

The bound of column j is the project's own per-transmission bound
(tests/test_gpu_channel.py: 1e-12 max(1, M_r) + 1e-12 |llr_r[j]|, M_r the
transmission's largest per-axis metric) summed over the transmissions that
carry j: each term is a transmission's own error, and the additions round the
same numbers in the same order on both sides.
"""
import numpy as np

import interleave_ref
from ldpc_amd.ratematch import KNOWN_LLR

SEED_STEP = 0x9E3779B97F4A7C15


def tx_seed(seed, r):
    return (int(seed) + r * SEED_STEP) % (1 << 64)


def frames_llr(spec, tx, shortened, block_len, c, seed, snr_point, sigma, frame0):
    """(llr [count, n], bound [count, n]) of the frames frame0 .. whose
    codewords are c under the plan tx (a sequence of column sequences), the
    shortened columns and the coherence length block_len."""
    c = np.asarray(c, np.uint8)
    count, n = c.shape
    llr = np.zeros((count, n), np.float64)
    bound = np.zeros((count, n), np.float64)
    for r, cols in enumerate(tx):
        cols = np.asarray(cols, np.int64)
        assert len(set(cols.tolist())) == len(cols) and cols.min() >= 0 and cols.max() < n
        assert not set(cols.tolist()) & set(shortened), "a plan column is shortened"
        for f in range(count):
            sent, M = interleave_ref.sent_llr(spec, c[f, cols], tx_seed(seed, r), frame0 + f, snr_point, sigma, block_len)
            llr[f, cols] = llr[f, cols] + sent
            bound[f, cols] += 1e-12 * max(1.0, M) + 1e-12 * np.abs(sent)
    llr[:, list(shortened)] = -KNOWN_LLR
    return llr, bound
