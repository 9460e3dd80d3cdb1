"""A numpy restatement of the fixed-point exit of the static 16-frame sub-tile
decoder (tile_sub_kernel<4>, csrc/tile_sub.hip), for tests.

It works from the states of a batch after passes 0 .. P-1, each the output of
a decode with max_iter = p + 1 and the exit off (the oracle's or the GPU's):
a dict with msgs [B, nnz] (CSR edge order), post [B, n] and conv [B].  A frame
that converged keeps its state from then on, as decode() returns it.

flags()   per pass and frame, what the kernel's verifying pass would find:
            pd  a posterior of an A column differs from the previous pass's
                (pass 0: from the channel value) -- the trigger, pdiffl;
            md  a message differs from the one it replaces -- mdiffl;
            nx  the next-pass proof fails for the frame: for some edge
                fl(L_old[col] - E_new) and fl(L_old[col] - E_old) differ in
                their bits, or an identity column's posterior changed.
          pass_flags() gives md and nx of one pass from two states.
replay()  the kernel's schedule per sub-tile of 16 consecutive frames (the
          trigger, vnext / vgap, the order of the exits, the back-off; one
          failed proof in a sub-tile voids the proof for that pass) and the
          pair that Decoder.fixed_point() reports: frames stopped at a fixed
          point, frame-passes they did not execute.  next_rule=False is the
          rule without the proof (LDPC_FP_NEXT=0).  With lazy=f, md and
          nx of pass `it` are asked of f(it) only where a sub-tile verifies
          (a long run needs the messages of few passes).
"""
import numpy as np

F = 16  # frames per workgroup


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def pass_flags(prev, cur, indices, k):
    """(md, nx), each bool [B], of the pass that maps state prev to state cur."""
    E0, L0, E1, L1 = prev["msgs"], prev["post"], cur["msgs"], cur["post"]
    B = len(E0)
    md, nx = np.zeros(B, bool), np.zeros(B, bool)
    for b in range(B):  # frame by frame: the gather is nnz doubles
        diff = _bits(E1[b]) != _bits(E0[b])
        md[b] = diff.any()
        e = np.flatnonzero(diff)  # where E repeats the two differences are the same expression
        Lg = L0[b, indices[e]]
        nx[b] = (_bits(Lg - E0[b, e]) != _bits(Lg - E1[b, e])).any() or \
            (_bits(L1[b, k:]) != _bits(L0[b, k:])).any()
    return md, nx


def flags(llr, states, indices, k):
    """(pd, md, nx), each bool [P, B].  md and nx of pass 0 are True (no
    verifying pass exists there)."""
    P, B = len(states), len(llr)
    pd = np.ones((P, B), bool)
    md = np.ones((P, B), bool)
    nx = np.ones((P, B), bool)
    pd[0] = (_bits(states[0]["post"][:, :k]) != _bits(llr[:, :k])).any(axis=1)
    for p in range(1, P):
        pd[p] = (_bits(states[p]["post"][:, :k]) != _bits(states[p - 1]["post"][:, :k])).any(axis=1)
        md[p], nx[p] = pass_flags(states[p - 1], states[p], indices, k)
    return pd, md, nx


class Horizon(Exception):
    """A frame still runs past the last pass whose state was given."""


def replay(pd, md, nx, conv, max_iter, next_rule=True, lazy=None):
    """(frames stopped at a fixed point, frame-passes not executed), and the
    pass at which each frame stopped (its last executed iteration)."""
    P, B = pd.shape
    stopped = skipped = 0
    last = np.full(B, -1, np.int64)
    for s in range(0, B, F):
        run = list(range(s, min(s + F, B)))
        trig, vnext, vgap = False, 1, 1
        for it in range(max_iter):
            if it >= P:
                raise Horizon(f"sub-tile {s // F}: frames {run} still run at iteration {it}")
            verify = it >= vnext and trig
            still, nfix = [], 0
            if lazy is not None:
                md_it, nx_it = lazy(it) if verify else (None, None)
            else:
                md_it, nx_it = md[it], nx[it]
            # the proof of a pass stands if it failed for no frame that entered the pass
            proved = verify and next_rule and not any(md_it[f] and nx_it[f] for f in run)
            for f in run:
                if conv[f] == it:  # syndrome zero: OK
                    last[f] = it
                elif it == max_iter - 1:
                    last[f] = it
                elif verify and not pd[it, f] and (not md_it[f] or proved):
                    last[f] = it
                    nfix += 1
                    skipped += max_iter - 1 - it
                else:
                    still.append(f)
            stopped += nfix
            trig = any(not pd[it, f] for f in still)
            run = still
            if not run:
                break
            if verify and nfix == 0:
                vnext = it + 1 + vgap
                vgap *= 2
    return (stopped, skipped), last
