"""HARQ plans of the physical-mode frame source (include/ldpc_hip.h, "HARQ"):
the transmissions a Decoder carries, their builders and the command line's
grammar.

A plan is R transmissions of one codeword.  Transmission r sends the columns of
its own list, in that order on the air, over an independent realisation of the
channel (its own noise and fades); the receiver adds the LLRs of every
transmission that carries a column.  Chase combining sends the same columns
again; incremental redundancy (IR) sends other columns of the mother code.

The builders read a circular buffer as rate matching in the cellular standards
does: the buffer is the non-shortened columns in ascending order (or a given
order), N of them; transmission r takes E consecutive buffer positions from
offset (r * step) mod N, wrapping at N.  step = 0 is Chase, step = E is IR.

Worked example: n = 576, no shortening, ir(576, 3, 384): the offsets are 0, 384
and 768 mod 576 = 192, so transmission 0 sends columns 0 .. 383, transmission 1
sends 384 .. 575 and then 0 .. 191 (a wrap), transmission 2 sends 192 .. 575:
after three transmissions every column has been sent twice.
"""
from dataclasses import dataclass, field

MAX_TX = 8  # LDPC_HARQ_MAX_TX
SEED_STEP = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def tx_seed(seed, r):
    """The Philox key of transmission r's noise and fade draws:
    (seed + r * 0x9E3779B97F4A7C15) mod 2^64; transmission 0 keeps `seed`."""
    return (int(seed) + int(r) * SEED_STEP) & _M64


@dataclass(frozen=True)
class HarqPlan:
    """An immutable tuple of column tuples, one per transmission, with the
    library's validation that needs no code (ldpc_harq_set): 1 .. MAX_TX
    transmissions, none empty, integer columns >= 0, none twice within one
    transmission.  validate(n, ...) adds what needs the code."""
    tx: tuple
    kind: str = "custom"
    params: dict = field(default_factory=dict, compare=False)

    def __post_init__(self):
        if isinstance(self.tx, (str, bytes)):
            raise ValueError(f"a HARQ plan is a sequence of column lists, got {self.tx!r}")
        try:
            lists = [list(t) for t in self.tx]
        except TypeError:
            raise ValueError("a HARQ plan is a sequence of column lists") from None
        if not 1 <= len(lists) <= MAX_TX:
            raise ValueError(f"a HARQ plan has 1 .. {MAX_TX} transmissions, got {len(lists)}")
        out = []
        for r, cols in enumerate(lists):
            try:
                vals = [int(c) for c in cols]
                same = all(v == c for v, c in zip(vals, cols))
            except (TypeError, ValueError):
                raise ValueError(f"transmission {r}: columns must be integers") from None
            if not same:
                raise ValueError(f"transmission {r}: columns must be integers")
            if not vals:
                raise ValueError(f"transmission {r} sends nothing (tx_len < 1)")
            if min(vals) < 0:
                raise ValueError(f"transmission {r}: column {min(vals)} is negative")
            if len(set(vals)) != len(vals):
                dup = next(c for i, c in enumerate(vals) if c in vals[:i])
                raise ValueError(f"transmission {r}: column {dup} is listed twice (duplicate)")
            out.append(tuple(vals))
        object.__setattr__(self, "tx", tuple(out))
        object.__setattr__(self, "params", dict(self.params))

    def __len__(self):
        return len(self.tx)

    @property
    def R(self):
        return len(self.tx)

    def n_sent(self, r):
        """E_r, the positions transmission r sends."""
        return len(self.tx[r])

    @property
    def lengths(self):
        return tuple(len(t) for t in self.tx)

    def truncated(self, R):
        """The plan of the first R transmissions."""
        if int(R) != R or not 1 <= int(R) <= len(self.tx):
            raise ValueError(f"truncated({R!r}): the plan has {len(self.tx)} transmissions")
        return HarqPlan(self.tx[:int(R)], self.kind, self.params)

    def validate(self, n, shortened=(), bps=None):
        """ValueError for what the library refuses on a code with n columns:
        a column outside [0, n), a column the pattern shortens, and (bps given)
        E_r % bps != 0."""
        n = int(n)
        short = set(int(c) for c in shortened)
        for r, cols in enumerate(self.tx):
            for c in cols:
                if c >= n:
                    raise ValueError(f"transmission {r}: column {c} is outside [0, {n})")
                if c in short:
                    raise ValueError(f"transmission {r} sends column {c}, which the pattern shortens")
            if bps is not None and len(cols) % int(bps) != 0:
                raise ValueError(f"transmission {r} sends E_r = {len(cols)} positions, not a multiple of bps = "
                                 f"{int(bps)}")
        return self

    def info(self):
        """The plan as a JSON document and the header line name it (no column lists)."""
        return {"kind": self.kind, "R": len(self.tx), "E": list(self.lengths), **self.params}

    @staticmethod
    def from_lists(lists):
        return HarqPlan(tuple(tuple(t) for t in lists), "custom")

    @staticmethod
    def circular(n, R, E, step, shortened=(), order=None, kind="circular"):
        """R transmissions of E positions each from the circular buffer (the
        module's head): offset (r * step) mod N.  ValueError for E > N (a column
        twice within one transmission), E < 1, R outside 1 .. MAX_TX, step < 0,
        or an `order` that is not the non-shortened columns exactly once."""
        n = int(n)
        short = set(int(c) for c in shortened)
        buf = [j for j in range(n) if j not in short]
        if order is not None:
            order = [int(c) for c in order]
            if sorted(order) != buf:
                raise ValueError("order must list every non-shortened column exactly once")
            buf = order
        N = len(buf)
        if int(R) != R or not 1 <= int(R) <= MAX_TX:
            raise ValueError(f"a HARQ plan has 1 .. {MAX_TX} transmissions, got R = {R!r}")
        if int(E) != E or int(E) < 1:
            raise ValueError(f"a transmission sends E >= 1 positions, got E = {E!r}")
        if int(E) > N:
            raise ValueError(f"E = {int(E)} > N = {N} buffer positions: a column would be sent twice in one transmission")
        if int(step) != step or int(step) < 0:
            raise ValueError(f"step must be an integer >= 0, got {step!r}")
        R, E, step = int(R), int(E), int(step)
        tx = tuple(tuple(buf[((r * step) % N + t) % N] for t in range(E)) for r in range(R))
        return HarqPlan(tx, kind, {"step": step, "buffer": N})

    @staticmethod
    def chase(n, R, E=None, shortened=(), order=None):
        """The same E positions R times (step = 0); E = None sends the whole buffer."""
        if E is None:
            E = int(n) - len(set(int(c) for c in shortened))
        return HarqPlan.circular(n, R, E, 0, shortened, order, kind="chase")

    @staticmethod
    def ir(n, R, E, shortened=(), order=None):
        """Consecutive windows of the buffer (step = E)."""
        return HarqPlan.circular(n, R, E, E, shortened, order, kind="ir")


def from_file(path):
    """One transmission per non-empty line: whitespace-separated column indices."""
    with open(path) as f:
        lines = [ln.split() for ln in f if ln.strip()]
    if not lines:
        raise ValueError(f"{path}: no transmissions")
    try:
        tx = tuple(tuple(int(t) for t in ln) for ln in lines)
    except ValueError:
        raise ValueError(f"{path}: columns must be integers") from None
    return HarqPlan(tx, "file", {"path": str(path)})


_FORMS = "chase:R[:E], ir:R:E or file:PATH"
_ARGS = {"chase": (1, 2), "ir": (2, 2)}


def split_spec(text):
    """(kind, arguments) of a command-line spec, its form checked without a
    code: integer arguments as ints, file's path as a string."""
    if not isinstance(text, str):
        raise ValueError(f"a HARQ spec is a string ({_FORMS}), got {type(text).__name__}")
    head, sep, rest = text.strip().partition(":")
    head = head.strip().lower()
    if head == "file":
        if not rest.strip():
            raise ValueError("HARQ spec file:PATH needs a path")
        return head, (rest,)
    if head not in _ARGS:
        raise ValueError(f"bad HARQ spec {text!r}: {_FORMS}")
    args = [a.strip() for a in rest.split(":")] if sep else []
    lo, hi = _ARGS[head]
    if not lo <= len(args) <= hi:
        raise ValueError(f"bad HARQ spec {text!r}: {_FORMS}")
    try:
        return head, tuple(int(a) for a in args)
    except ValueError:
        raise ValueError(f"bad HARQ spec {text!r}: R and E are integers") from None


def parse(text, n, shortened=()):
    """The command line's forms, resolved against a code with n columns and the
    pattern's shortened columns: chase:R[:E], ir:R:E, file:PATH."""
    head, args = split_spec(text)
    if head == "file":
        return from_file(args[0]).validate(n, shortened)
    if head == "chase":
        return HarqPlan.chase(n, args[0], args[1] if len(args) > 1 else None, shortened)
    return HarqPlan.ir(n, args[0], args[1], shortened)


HarqPlan.parse = staticmethod(parse)


def resolve(plan, n, shortened=()):
    """simulate_harq()'s argument -- a HarqPlan or a spec string -- as a
    HarqPlan valid for the code."""
    if isinstance(plan, HarqPlan):
        return plan.validate(n, shortened)
    if isinstance(plan, str):
        return parse(plan, n, shortened)
    raise ValueError(f"harq must be a HarqPlan or a spec string, got {type(plan).__name__}")
