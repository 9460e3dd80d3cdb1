"""Rate matching of the physical-mode frame source (include/ldpc_hip.h, "rate
matching"): the pattern a Decoder carries, its effective rate, and the command
line's column grammar.

A column (in the frame's order: info 0 .. k-1, parity k .. n-1) is transmitted,
punctured (not sent, unknown to the receiver: llr = +0.0) or shortened (an
information bit both ends know to be 0, not sent: llr = -KNOWN_LLR).  The
transmitted columns in ascending order are what the channel model maps to
symbols; E = n - n_punct - n_short of them, carrying k - n_short information
bits, so the effective rate is (k - n_short) / E.

Worked example: wimax_2304_0.5 (k = 1152) with every sixth parity column
punctured, "k:n:6": 192 columns, E = 2112, rate 1152 / 2112 = 0.545.
"""
import re
from dataclasses import dataclass

KNOWN_LLR = 1.0e4  # LDPC_RM_KNOWN_LLR


@dataclass(frozen=True)
class RateMatch:
    """{punctured, shortened} column tuples (kept ascending) with the library's
    validation (ldpc_rate_match_set), raised as ValueError before any device
    call once the code's n and k are known (validate)."""
    punctured: tuple = ()
    shortened: tuple = ()

    def __post_init__(self):
        for name in ("punctured", "shortened"):
            cols = getattr(self, name)
            if isinstance(cols, (str, bytes)):
                raise ValueError(f"{name} must be a sequence of column indices, got {cols!r}")
            try:
                vals = [int(c) for c in cols]
                same = all(v == c for v, c in zip(vals, cols))
            except (TypeError, ValueError):
                raise ValueError(f"{name} must be a sequence of integer column indices") from None
            if not same:
                raise ValueError(f"{name} must be a sequence of integer column indices")
            object.__setattr__(self, name, tuple(sorted(vals)))

    @property
    def is_empty(self):
        return not self.punctured and not self.shortened

    def validate(self, n, k, bps=None):
        """ValueError for what ldpc_rate_match_set refuses on an (n, k) code,
        and (bps given) for E % bps != 0, which generating frames refuses."""
        n, k = int(n), int(k)
        seen = set()
        for name, cols in (("punctured", self.punctured), ("shortened", self.shortened)):
            for c in cols:
                if not 0 <= c < n:
                    raise ValueError(f"{name} column {c} is outside [0, {n})")
                if c in seen:
                    raise ValueError(f"column {c} is listed twice (duplicate)")
                seen.add(c)
        for c in self.shortened:
            if c >= k:
                raise ValueError(f"shortened column {c} is not an information column (k = {k})")
        E = n - len(seen)
        if E < 1:
            raise ValueError("no transmitted column is left (E < 1)")
        if k - len(self.shortened) < 1:
            raise ValueError("no information bit is left (k - n_short < 1)")
        if bps is not None and not self.is_empty and E % int(bps) != 0:
            raise ValueError(f"E = {E} transmitted bits is not a multiple of bps = {int(bps)}")
        return self

    def transmitted(self, n):
        """The transmitted columns, ascending (E of them)."""
        out = set(self.punctured) | set(self.shortened)
        return [j for j in range(int(n)) if j not in out]

    def n_transmitted(self, n):
        return int(n) - len(set(self.punctured) | set(self.shortened))

    def info_bits(self, k):
        return int(k) - len(self.shortened)

    def effective_rate(self, n, k):
        """(k - n_short) / E: the rate the Eb/N0 axis and the config report."""
        return self.info_bits(k) / self.n_transmitted(n)

    def info(self, n, k):
        """The pattern as --stats-json writes it."""
        return {"punctured": list(self.punctured), "shortened": list(self.shortened),
                "transmitted": self.n_transmitted(n), "info_bits": self.info_bits(k),
                "rate": self.effective_rate(n, k)}


_BOUND = re.compile(r"^\s*(?:([kn])\s*(?:([+-])\s*(\d+))?|([+-]?\d+))\s*$")


def _bound(text, n, k):
    m = _BOUND.match(text)
    if not m:
        raise ValueError(f"bad column bound {text!r}: an integer, or k / n optionally followed by +INT / -INT")
    if m.group(4) is not None:
        return int(m.group(4))
    base = int(k) if m.group(1) == "k" else int(n)
    return base + (int(m.group(3)) if m.group(2) == "+" else -int(m.group(3))) if m.group(2) else base


def parse_columns(text, n, k):
    """Columns of the command line's grammar, ascending and without repeats:
    comma-separated items `a`, `a:b`, `a:b:step`, half-open as Python slices
    (no negative indices: a bound counts from 0); a bound is an integer, or
    k / n optionally followed by +INT / -INT.  "k:n:6", "0:24", "n-48:n".
    ValueError for anything else, an empty item, a step < 1, or a column
    outside [0, n)."""
    n, k = int(n), int(k)
    cols = []
    if text is None or not str(text).strip():
        raise ValueError("empty column list")
    for item in str(text).split(","):
        parts = item.split(":")
        if not item.strip() or len(parts) > 3 or any(not p.strip() for p in parts):
            raise ValueError(f"bad column item {item!r}: a, a:b or a:b:step")
        if len(parts) == 1:
            got = [_bound(parts[0], n, k)]
        else:
            a, b = _bound(parts[0], n, k), _bound(parts[1], n, k)
            step = 1
            if len(parts) == 3:
                if not re.fullmatch(r"\s*\d+\s*", parts[2]) or int(parts[2]) < 1:
                    raise ValueError(f"bad step in {item!r}: a positive integer")
                step = int(parts[2])
            if a < 0 or b < 0:
                raise ValueError(f"negative bound in {item!r}")
            got = list(range(a, b, step))
        for c in got:
            if not 0 <= c < n:
                raise ValueError(f"column {c} of {item!r} is outside [0, {n})")
        cols.extend(got)
    if len(set(cols)) != len(cols):
        raise ValueError(f"a column is listed twice in {text!r}")
    return tuple(sorted(cols))
