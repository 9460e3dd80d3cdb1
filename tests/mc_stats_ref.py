"""CPU restatement of the physical-mode Monte-Carlo statistics
(ldpc_mc_stats_read, include/ldpc_hip.h) on a decoder restatement's per-frame
results (minsum_ref / qminsum_ref / phys_decode: z, conv, status), plus the
identities that tie a histogram to the counters row of the same run."""
import numpy as np


def stats(u, o, T, frame0=0):
    """The dict Decoder.mc_stats_read returns with max_failed = len(u) for the
    frames whose info bits are u [B, k] and whose decode gave o (z = bit
    estimate ^ 1, conv, status), the first frame's global index frame0."""
    u = np.asarray(u, dtype=np.uint8)
    k = u.shape[1]
    ok = np.asarray(o["status"]) == 0
    conv = np.asarray(o["conv"])
    err = ((np.asarray(o["z"])[:, :k] ^ 1).astype(np.uint8) != u).sum(axis=1).astype(np.int64)
    hist = np.zeros(T + 1, np.int64)
    hist[:T] = np.bincount(conv[ok], minlength=T)[:T]
    hist[T] = int((~ok).sum())
    und = ok & (err > 0)
    idx = np.nonzero(~ok)[0].astype(np.int64)
    return {"hist": hist, "undetected_frames": int(und.sum()), "undetected_bit_errors": int(err[und].sum()),
            "failed": np.stack([frame0 + idx, err[idx]], axis=1).reshape(-1, 2), "failed_dropped": 0}


def assert_identities(hist, c):
    """The five identities between hist [T + 1] and the counters row c [7]."""
    hist = np.asarray(hist, dtype=np.int64)
    T = len(hist) - 1
    t = np.arange(T, dtype=np.int64)
    assert int(hist.sum()) == int(c[0]), "sum(hist) == frames"
    assert int(hist[T]) == int(c[1]), "hist[T] == failed"
    assert int(hist[:T].sum()) == int(c[4]), "converged frames"
    assert int((t * hist[:T]).sum()) == int(c[3]), "sum of conv"
    assert int(((t + 1) * hist[:T]).sum()) + T * int(hist[T]) == int(c[6]), "iterations"


def assert_equal(got, want, what=""):
    """Two statistics dicts are the same, field by field."""
    np.testing.assert_array_equal(got["hist"], want["hist"], err_msg=f"{what}: hist")
    assert (got["undetected_frames"], got["undetected_bit_errors"]) == \
        (want["undetected_frames"], want["undetected_bit_errors"]), f"{what}: undetected"
    np.testing.assert_array_equal(got["failed"], want["failed"], err_msg=f"{what}: failed")
    assert got["failed_dropped"] == want["failed_dropped"], f"{what}: failed_dropped"
