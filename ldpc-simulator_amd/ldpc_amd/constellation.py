"""Constellation tables of the physical-mode frame source (include/ldpc_hip.h,
"constellations"): 2^bps complex points indexed by label, which replace the
channel's square Gray QAM while they are set on a Decoder.

Label a of a symbol: its bits, the first the most significant.  The frame
source sends points[a] and demaps over all 2^bps points, so any labelling and
any shape can be written down: PSK, APSK, cross or rotated QAM.  sigma keeps
its meaning (Es/N0 = 1 / (2 sigma^2)) because a table has unit mean energy.

The built-in tables are this project's own, stated here in full.  They claim no
conformity with any standard: gamma = 3.15 is a commonly quoted ring ratio, not
checked against one, and the labellings are simply Gray-like ones that are easy
to write down.  Whoever has a standard's table loads it with from_file.

  psk8()       unit circle; label a0a1a2 -> B = a ^ (a >> 1) ^ (a >> 2) (the Gray
               decoding rule of the QAM axes), angle (2B + 1) pi / 8, so that
               neighbours on the circle differ in one bit, the wrap included
  apsk16(g)    4 + 12 points, g = R2 / R1 > 1, R1 = sqrt(16 / (4 + 12 g^2)).
               First quadrant by a0a1: 00 -> R2 e^(i pi/4), 01 -> R2 e^(i pi/12),
               10 -> R2 e^(i 5pi/12), 11 -> R1 e^(i pi/4); a2 = 1 negates the real
               part, a3 = 1 the imaginary part
"""
import cmath
import math
from dataclasses import dataclass

MAX_BPS = 6          # LDPC_CONST_MAX_BPS
ENERGY_TOL = 1e-9    # |mean |x|^2 - 1| the library accepts


@dataclass(frozen=True)
class Constellation:
    """{name, points} with the library's validation (ldpc_constellation_set),
    raised as ValueError before any device call.  points: a tuple of 2^bps
    complex numbers, indexed by label."""
    name: str
    points: tuple

    def __post_init__(self):
        try:
            pts = tuple(complex(p) for p in self.points)
        except (TypeError, ValueError) as e:
            raise ValueError(f"constellation points must be complex numbers: {e}") from None
        object.__setattr__(self, "points", pts)
        object.__setattr__(self, "name", str(self.name))
        n = len(pts)
        if n < 2 or n > (1 << MAX_BPS) or n & (n - 1):
            raise ValueError(f"a constellation has 2^bps points, 1 <= bps <= {MAX_BPS}; got {n}")
        for i, p in enumerate(pts):
            if not (math.isfinite(p.real) and math.isfinite(p.imag)):
                raise ValueError(f"constellation point {i} has a coordinate that is not finite")
        energy = sum(p.real * p.real + p.imag * p.imag for p in pts) / n
        if not abs(energy - 1.0) <= ENERGY_TOL:
            raise ValueError(f"the mean energy of the {n} points is {energy:.12g}, not 1 to within {ENERGY_TOL:g} "
                             "(from_points(..., normalize=True) scales a table)")
        seen = {}
        for i, p in enumerate(pts):
            if p in seen:
                raise ValueError(f"constellation points {seen[p]} and {i} are equal")
            seen[p] = i

    @property
    def bps(self):
        return len(self.points).bit_length() - 1

    def flat(self):
        """[re0, im0, re1, im1, ...] as the C ABI takes the table."""
        return [c for p in self.points for c in (p.real, p.imag)]

    def info(self):
        """The table as --stats-json / --harq-json write it."""
        return {"name": self.name, "bps": self.bps, "points": [[p.real, p.imag] for p in self.points]}

    def check_length(self, n):
        """ValueError when n transmitted bits do not divide into symbols."""
        if int(n) % self.bps != 0:
            raise ValueError(f"n = {int(n)} is not a multiple of bps = {self.bps} (constellation {self.name})")

    @classmethod
    def psk8(cls):
        pts = []
        for a in range(8):
            B = (a ^ (a >> 1) ^ (a >> 2)) & 7
            pts.append(cmath.exp(1j * (2 * B + 1) * math.pi / 8.0))
        return cls("8psk", tuple(pts))

    @classmethod
    def apsk16(cls, gamma=3.15):
        gamma = float(gamma)
        if not (math.isfinite(gamma) and gamma > 1.0):
            raise ValueError(f"16apsk: gamma = R2 / R1 must be a finite number > 1, got {gamma!r}")
        r1 = math.sqrt(16.0 / (4.0 + 12.0 * gamma * gamma))
        r2 = gamma * r1
        quad = (r2 * cmath.exp(1j * math.pi / 4.0), r2 * cmath.exp(1j * math.pi / 12.0),
                r2 * cmath.exp(1j * 5.0 * math.pi / 12.0), r1 * cmath.exp(1j * math.pi / 4.0))
        pts = []
        for a in range(16):
            q = quad[a >> 2]
            pts.append(complex(-q.real if a & 2 else q.real, -q.imag if a & 1 else q.imag))
        return cls("16apsk" if gamma == 3.15 else f"16apsk:{gamma:g}", tuple(pts))

    @classmethod
    def from_points(cls, points, name="custom", normalize=True):
        """A table from a list of 2^bps complex points; normalize scales it to
        unit mean energy (else it must have it already)."""
        try:
            pts = [complex(p) for p in points]
        except (TypeError, ValueError) as e:
            raise ValueError(f"constellation points must be complex numbers: {e}") from None
        if normalize and pts:
            if not all(math.isfinite(p.real) and math.isfinite(p.imag) for p in pts):
                raise ValueError("a constellation point has a coordinate that is not finite")
            energy = sum(p.real * p.real + p.imag * p.imag for p in pts) / len(pts)
            if not energy > 0.0:
                raise ValueError("a constellation of zero energy cannot be normalised")
            s = 1.0 / math.sqrt(energy)
            pts = [p * s for p in pts]
        return cls(name, tuple(pts))

    @classmethod
    def from_file(cls, path, name=None, normalize=False):
        """A table from a text file: one `re im` pair per line, the line index
        (comments and blank lines not counted) is the label, `#` starts a
        comment.  The table must have unit mean energy unless normalize."""
        pts = []
        try:
            with open(path) as f:
                for ln, line in enumerate(f, 1):
                    line = line.split("#", 1)[0].split()
                    if not line:
                        continue
                    if len(line) != 2:
                        raise ValueError(f"{path}:{ln}: expected `re im`, got {len(line)} fields")
                    try:
                        pts.append(complex(float(line[0]), float(line[1])))
                    except ValueError:
                        raise ValueError(f"{path}:{ln}: `{' '.join(line)}` is not a pair of numbers") from None
        except OSError as e:
            raise ValueError(f"constellation file: {e}") from None
        return cls.from_points(pts, name=name or f"file:{path}", normalize=normalize)

    def to_file(self, path):
        """Write the table as from_file reads it (17 significant digits: the
        doubles round-trip)."""
        with open(path, "w") as f:
            f.write(f"# {self.name}: {len(self.points)} points, re im, line index = label\n")
            for p in self.points:
                f.write(f"{p.real!r} {p.imag!r}\n")


def parse(spec):
    """The command line's --constellation value: 8psk | 16apsk[:GAMMA] |
    file:PATH.  ValueError otherwise (the ChannelSpec-style spelling psk8 is not
    a name here either)."""
    s = str(spec).strip()
    low = s.lower()
    if low == "8psk":
        return Constellation.psk8()
    if low == "16apsk":
        return Constellation.apsk16()
    if low.startswith("16apsk:"):
        try:
            gamma = float(s.split(":", 1)[1])
        except ValueError:
            raise ValueError(f"--constellation 16apsk:GAMMA takes a number, got {s!r}") from None
        return Constellation.apsk16(gamma)
    if low.startswith("file:"):
        return Constellation.from_file(s[5:])
    raise ValueError(f"constellation must be 8psk, 16apsk[:GAMMA] or file:PATH, got {spec!r}")


def effective_bps(channel, constellation):
    """Bits per symbol of the frames: the table's while one is set."""
    return constellation.bps if constellation is not None else channel.bps
