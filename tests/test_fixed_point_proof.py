"""The next-pass proof of the static sub-tile decoder's fixed-point exit
(csrc/tile_sub.hip, restated in fixed_point_ref.py), checked on the CPU oracle.

Pass p maps (E_old, L_old) to (E_new, L_new).  If L_new == L_old bit for bit on
every column and, for every edge, fl(L_old[col] - E_new) has the bits of
fl(L_old[col] - E_old), pass p + 1 forms the variable-to-check values of pass p
and so reproduces (E_new, L_new): the frame sits at a fixed point from pass p
on, although E_new != E_old.  Here: wherever the proof holds on the oracle's
states after passes 0 .. 4 (T = 1 .. 5), every later state equals the proven
one bit for bit -- no counterexample -- and the frames for which the proof adds
something over "no message differed" exist, so that the GPU tests built on them
cannot pass vacuously.

Frames: the on-device source restated by the oracle, seed 20260213, wimax_2304_0.5.
"""
import numpy as np
import pytest

import fixed_point_ref as ref
import oracle
from conftest import hstd_for

CODE = "wimax_2304_0.5"
SEED = 20260213
FRAME0 = 32768
P = 5


def _states(snr, frame0):
    H = hstd_for(CODE)
    _, _, llr = oracle.generate_frames(H, SEED, 0, oracle.sigma_for_snr(snr), frame0, 64)
    states = [oracle.spa_decode(H, llr, T, want_E=True) for T in range(1, P + 1)]
    return H, llr, states


_CASES = {"1dB": (1.0, FRAME0 + 256), "2dB": (2.0, FRAME0)}
_DONE = {}


def _case(name):
    """(states, pd, md, nx) of a set of 64 frames: decoded once."""
    if name not in _DONE:
        H, llr, states = _states(*_CASES[name])
        k = H.shape[1] - H.shape[0]
        _DONE[name] = (states,) + ref.flags(llr, states, np.asarray(H.indices), k)
    return _DONE[name]


def _same(a, b, f):
    return np.array_equal(ref._bits(a["msgs"][f]), ref._bits(b["msgs"][f])) and \
        np.array_equal(ref._bits(a["post"][f]), ref._bits(b["post"][f]))


@pytest.mark.parametrize("snr", list(_CASES))
def test_no_counterexample(snr):
    states, pd, md, nx = _case(snr)
    conv = states[-1]["conv"]
    held = extra = 0
    for p in range(1, P - 1):
        for f in range(64):
            if 0 <= conv[f] <= p:  # converged: its state is frozen, nothing to prove
                continue
            if pd[p, f] or nx[p, f]:
                continue
            held += 1
            extra += bool(md[p, f])
            for q in range(p + 1, P):
                assert _same(states[q], states[p], f), f"{snr}: frame {f}, proof at pass {p}, state after pass {q} differs"
    print(f"{snr}: proof held {held} times, {extra} of them with messages that differed")
    if snr == "1dB":  # at 2 dB no frame has settled by pass 3
        assert held > 0 and extra > 0


@pytest.mark.parametrize("snr", list(_CASES))
def test_no_message_differed_is_a_special_case(snr):
    _, pd, md, nx = _case(snr)
    assert not (nx[1:] & ~md[1:]).any()


def test_stragglers_exist_at_1db():
    """Frames 32768 + 256 and + 262: their posteriors repeat in pass 2 (L3 == L2)
    but their messages do not (E3 != E2), and the proof holds there."""
    states, pd, md, nx = _case("1dB")
    for f in (0, 6):
        assert np.array_equal(ref._bits(states[2]["post"][f]), ref._bits(states[1]["post"][f]))
        assert not np.array_equal(ref._bits(states[2]["msgs"][f]), ref._bits(states[1]["msgs"][f]))
        assert not pd[2, f] and md[2, f] and not nx[2, f]
