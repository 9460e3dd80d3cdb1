"""Bit interleavers of the physical-mode frame source (include/ldpc_hip.h, "bit
interleaver and block fading"): the permutation a Decoder carries, its builders
and the command line's grammar.

Let tx[0 .. E-1] be the transmitted columns in ascending order (every column,
E = n, without a rate-matching pattern).  An interleaver is a permutation pi of
0 .. E-1, read-from: transmitted position t carries column tx[pi[t]], so the
bits of one symbol -- and, under block fading, of one fade -- are columns that
pi brings together.  The frame source writes the LLR of position t back to that
column; the decoders never see the permutation.

The reference (python_ldpc_app/interleavers.py) has the same three kinds.  Its
regular interleaver is `regular` here, shape rule included.  Its random and
S-random interleavers draw a fresh permutation for every frame from Python's
global generator; ours is ONE permutation, fixed for a run, as in a real link
where both ends agree on it beforehand -- and drawn from a generator written
out below (splitmix64), so (E, seed) names the same permutation on every
machine and library version.

Worked example: E = 6, block(6, 2): the positions are written by rows into 2
rows of 3 and read by columns, pi = [0, 3, 1, 4, 2, 5]; with QPSK symbol 0
carries columns 0 and 3, symbol 1 carries 1 and 4, symbol 2 carries 2 and 5.
"""
import math
from dataclasses import dataclass, field

_M64 = (1 << 64) - 1
SRANDOM_RESTARTS = 64


class SplitMix64:
    """state += 0x9E3779B97F4A7C15; z = state; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
    z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31 -- all mod 2^64, the
    state starting at `seed`.  The first value at seed 0 is 0xE220A8397B1DCDAF."""

    def __init__(self, seed=0):
        self.state = int(seed) & _M64

    def next(self):
        self.state = (self.state + 0x9E3779B97F4A7C15) & _M64
        z = self.state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
        return z ^ (z >> 31)


def _shuffle(vals, gen):
    """Fisher-Yates in place: for i = len-1 down to 1, j = next() mod (i+1), swap i and j."""
    for i in range(len(vals) - 1, 0, -1):
        j = gen.next() % (i + 1)
        vals[i], vals[j] = vals[j], vals[i]
    return vals


@dataclass(frozen=True)
class Interleaver:
    """A permutation (read-from) with the name and parameters it was built
    from.  The library's validation (ldpc_interleaver_set) is raised here as
    ValueError; validate(E) adds the length check that generating frames makes."""
    perm: tuple
    kind: str = "custom"
    params: dict = field(default_factory=dict, compare=False)

    def __post_init__(self):
        if isinstance(self.perm, (str, bytes)):
            raise ValueError(f"perm must be a sequence of integers, got {self.perm!r}")
        try:
            vals = [int(v) for v in self.perm]
            same = all(v == p for v, p in zip(vals, self.perm))
        except (TypeError, ValueError):
            raise ValueError("perm must be a sequence of integers") from None
        if not same:
            raise ValueError("perm must be a sequence of integers")
        E = len(vals)
        seen = bytearray(E)
        for v in vals:
            if not 0 <= v < E:
                raise ValueError(f"entry {v} is outside [0, {E})")
            if seen[v]:
                raise ValueError(f"entry {v} is listed twice (duplicate)")
            seen[v] = 1
        object.__setattr__(self, "perm", tuple(vals))
        object.__setattr__(self, "params", dict(self.params))

    def __len__(self):
        return len(self.perm)

    @property
    def is_identity(self):
        return all(v == t for t, v in enumerate(self.perm))

    def validate(self, E):
        """ValueError unless the permutation has the E entries a code (under
        its rate-matching pattern) transmits."""
        if len(self.perm) != int(E):
            raise ValueError(f"the interleaver has length {len(self.perm)}, the frames transmit E = {int(E)} bits")
        return self

    def info(self):
        """The interleaver as --stats-json writes it (no permutation: kind,
        parameters and length rebuild it, except for file / custom ones)."""
        return {"kind": self.kind, "length": len(self.perm), **self.params}


def _length(E):
    if int(E) != E or int(E) < 1:
        raise ValueError(f"an interleaver needs a length E >= 1, got {E!r}")
    return int(E)


def identity(E):
    E = _length(E)
    return Interleaver(tuple(range(E)), "identity")


def block(E, rows):
    """Written by rows into rows x C (C = E / rows), read by columns:
    pi[c * rows + r] = r * C + c.  rows must divide E."""
    E = _length(E)
    if int(rows) != rows or int(rows) < 1 or E % int(rows) != 0:
        raise ValueError(f"block interleaver: rows = {rows!r} must be a positive divisor of E = {E}")
    rows = int(rows)
    C = E // rows
    return Interleaver(tuple(r * C + c for c in range(C) for r in range(rows)), "block", {"rows": rows, "cols": C})


def regular_shape(E):
    """The reference's shape rule: rows = the largest divisor of E that is <=
    floor(sqrt(E)); 576 -> 24 x 24, 504 -> 21 x 24, a prime E -> 1 x E."""
    E = _length(E)
    rows = math.isqrt(E)
    while E % rows:
        rows -= 1
    return rows, E // rows


def regular(E):
    """block(E, rows) with the reference's shape (regular_shape)."""
    rows, cols = regular_shape(E)
    b = block(E, rows)
    return Interleaver(b.perm, "regular", {"rows": rows, "cols": cols})


def random(E, seed=0):
    """Fisher-Yates from the identity with SplitMix64(seed)."""
    E = _length(E)
    return Interleaver(tuple(_shuffle(list(range(E)), SplitMix64(seed))), "random", {"seed": int(seed)})


def s_distance_ok(perm, S):
    """|perm[i] - perm[j]| > S whenever 0 < |i - j| <= S."""
    return all(abs(perm[i] - perm[j]) > S for i in range(len(perm)) for j in range(max(0, i - S), i))


def srandom(E, S, seed=0):
    """An S-random permutation: |pi[i] - pi[j]| > S whenever 0 < |i - j| <= S.
    One SplitMix64(seed) stream serves every attempt.  An attempt shuffles
    0 .. E-1 (Fisher-Yates as `random`) into a candidate list and fills the
    positions in order: position i takes the first candidate left in the list
    that is more than S away from each of the S values before it.  When no
    candidate fits, the attempt is dropped and the next one starts with a new
    shuffle from the same stream; after SRANDOM_RESTARTS (64) dropped attempts
    construction gives up.  ValueError then, and for S > floor(sqrt(E / 2)),
    beyond which the construction is not expected to end.  S = 0 is `random`."""
    E = _length(E)
    if int(S) != S or int(S) < 0:
        raise ValueError(f"S-random interleaver: S = {S!r} must be an integer >= 0")
    S = int(S)
    if S > math.isqrt(E // 2):
        raise ValueError(f"S-random interleaver: S = {S} > floor(sqrt(E / 2)) = {math.isqrt(E // 2)} for E = {E}")
    gen = SplitMix64(seed)
    for _ in range(SRANDOM_RESTARTS):
        cand = _shuffle(list(range(E)), gen)
        perm = []
        for i in range(E):
            recent = perm[max(0, i - S):]
            for ci, c in enumerate(cand):
                if all(abs(c - p) > S for p in recent):
                    perm.append(cand.pop(ci))
                    break
            else:
                break
        if len(perm) == E:
            return Interleaver(tuple(perm), "srandom", {"S": S, "seed": int(seed)})
    raise ValueError(f"S-random interleaver: no permutation after {SRANDOM_RESTARTS} attempts (E = {E}, S = {S}, "
                     f"seed = {int(seed)})")


def from_file(path):
    """E whitespace-separated integers, a permutation of 0 .. E-1."""
    with open(path) as f:
        text = f.read().split()
    if not text:
        raise ValueError(f"{path}: no permutation entries")
    try:
        vals = tuple(int(t) for t in text)
    except ValueError:
        raise ValueError(f"{path}: entries must be integers") from None
    return Interleaver(vals, "file", {"path": str(path)})


_FORMS = "none, regular, block:R, random[:seed], srandom:S[:seed] or file:PATH"
_ARGS = {"none": (0, 0), "regular": (0, 0), "block": (1, 1), "random": (0, 1), "srandom": (1, 2)}


def split_spec(text):
    """(kind, arguments) of a command-line spec, its form checked without a
    length: the kinds of parse(), integer arguments as ints, file's path as a
    string.  ValueError for anything else."""
    if not isinstance(text, str):
        raise ValueError(f"an interleaver spec is a string ({_FORMS}), got {type(text).__name__}")
    head, sep, rest = text.strip().partition(":")
    head = head.strip().lower()
    if head == "file":
        if not rest.strip():
            raise ValueError("interleaver spec file:PATH needs a path")
        return head, (rest,)
    if head not in _ARGS:
        raise ValueError(f"bad interleaver spec {text!r}: {_FORMS}")
    args = [a.strip() for a in rest.split(":")] if sep else []
    lo, hi = _ARGS[head]
    if not lo <= len(args) <= hi:
        raise ValueError(f"bad interleaver spec {text!r}: {_FORMS}")
    try:
        return head, tuple(int(a) for a in args)
    except ValueError:
        raise ValueError(f"bad interleaver spec {text!r}: R, S and seed are integers") from None


def parse(text, E):
    """The command line's forms, resolved against E transmitted bits: none,
    regular, block:R, random[:seed], srandom:S[:seed], file:PATH.  None for
    `none`; ValueError for anything else the grammar or a builder refuses."""
    head, args = split_spec(text)
    if head == "none":
        return None
    if head == "file":
        return from_file(args[0]).validate(E)
    return {"regular": regular, "block": block, "random": random, "srandom": srandom}[head](E, *args)


def resolve(il, E):
    """simulate()'s argument -- None, an Interleaver or a spec string -- as an
    Interleaver of length E, or None."""
    if il is None:
        return None
    if isinstance(il, Interleaver):
        return il.validate(E)
    if isinstance(il, str):
        return parse(il, E)
    raise ValueError(f"interleaver must be an Interleaver, a spec string or None, got {type(il).__name__}")
