"""Channel models of the physical-mode frame source (include/ldpc_hip.h,
"channel models"): the spec a Decoder carries, and the SNR axes.

The reference channel (the default) is the reference simulator's mode 1 as the
frame source has always restated it: BPSK, noise standard deviation sigma^2,
llr = 2y/sigma^2, and an SNR axis without a code-rate term
(montecarlo.sigma_for_snr).  "awgn" and "rayleigh" are the textbook models:
sigma is the noise standard deviation per real dimension at unit average symbol
energy, so Es/N0 = 1 / (2 sigma^2) for every modulation and
Eb/N0 = Es/N0 / (rate * bps).

Worked example of the reference axis: its "-2.5 dB" point has
sigma = 1/sqrt(2 * 10^-0.25) = 0.943, and the noise standard deviation is
sigma^2 = 0.889; a textbook BPSK channel with that noise has
Es/N0 = 1 / (2 * 0.889^2) = -1.99 dB, which at rate 1/2 is Eb/N0 = +1.02 dB
(reference_axis_as_ebn0).
"""
import math
from dataclasses import dataclass

MODELS = {"reference": 0, "awgn": 1, "rayleigh": 2}      # LDPC_CH_*
MODULATIONS = {"bpsk": 1, "qpsk": 2, "qam16": 4, "qam64": 6}  # bits per symbol
DEMAPS = {"exact": 0, "maxlog": 1}                        # LDPC_DEMAP_*
SNR_AXES = ("reference", "esn0", "ebn0")


@dataclass(frozen=True)
class ChannelSpec:
    """{model, modulation, demap} with the library's validation
    (ldpc_channel_set), raised as ValueError before any device call."""
    model: str = "reference"
    modulation: str = "bpsk"
    demap: str = "exact"

    def __post_init__(self):
        if self.model not in MODELS:
            raise ValueError(f"channel model must be one of {sorted(MODELS)}, got {self.model!r}")
        if self.modulation not in MODULATIONS:
            raise ValueError(f"modulation must be one of {sorted(MODULATIONS)}, got {self.modulation!r}")
        if self.demap not in DEMAPS:
            raise ValueError(f"demap must be one of {sorted(DEMAPS)}, got {self.demap!r}")
        if self.model == "reference" and self.modulation != "bpsk":
            raise ValueError(f"the reference channel is BPSK only, got modulation {self.modulation!r}")

    @property
    def bps(self):
        return MODULATIONS[self.modulation]

    @property
    def is_reference(self):
        return self.model == "reference"

    def codes(self):
        """(model, modulation, demap) as the C ABI's integers."""
        return MODELS[self.model], self.bps, DEMAPS[self.demap]

    @classmethod
    def from_codes(cls, model, modulation, demap):
        inv = [{v: k for k, v in t.items()} for t in (MODELS, MODULATIONS, DEMAPS)]
        return cls(inv[0][int(model)], inv[1][int(modulation)], inv[2][int(demap)])

    def check_length(self, n):
        """ValueError when a code of length n does not divide into symbols."""
        if not self.is_reference and int(n) % self.bps != 0:
            raise ValueError(f"n = {int(n)} is not a multiple of bps = {self.bps} ({self.modulation})")


def sigma_for_esn0(esn0_db):
    """Noise standard deviation per real dimension at Es/N0 (dB), Es = 1."""
    return math.sqrt(1.0 / (2.0 * 10.0 ** (float(esn0_db) / 10.0)))


def sigma_for_ebn0(ebn0_db, rate, bps, table=False):
    """The same at Eb/N0 (dB) for a code of rate `rate` on `bps` bits per symbol:
    Es = rate * bps * Eb.  bps is a built-in modulation's, or with table=True a
    constellation table's (1 .. 6)."""
    rate, bps = float(rate), int(bps)
    if not 0.0 < rate <= 1.0:
        raise ValueError(f"rate must be in (0, 1], got {rate}")
    if table:
        if not 1 <= bps <= 6:
            raise ValueError(f"a constellation table's bps must be in 1 .. 6, got {bps}")
    elif bps not in MODULATIONS.values():
        raise ValueError(f"bps must be one of {sorted(MODULATIONS.values())}, got {bps}")
    return math.sqrt(1.0 / (2.0 * rate * bps * 10.0 ** (float(ebn0_db) / 10.0)))


def reference_axis_as_ebn0(snr_db, rate):
    """(noise standard deviation, Es/N0 dB, Eb/N0 dB) of the reference
    channel's SNR point read as a textbook BPSK channel: its noise standard
    deviation is sigma^2 with sigma = 1/sqrt(2 * 10^(snr/10))."""
    std = 1.0 / (2.0 * 10.0 ** (float(snr_db) / 10.0))
    esn0 = 10.0 * math.log10(1.0 / (2.0 * std * std))
    return std, esn0, esn0 - 10.0 * math.log10(float(rate))


def resolve_snr_axis(spec, snr_axis=None):
    """The axis a sweep under `spec` uses: the reference channel has only its
    own; the models default to "ebn0".  ValueError otherwise."""
    spec = spec or ChannelSpec()
    if snr_axis is None:
        snr_axis = "reference" if spec.is_reference else "ebn0"
    if snr_axis not in SNR_AXES:
        raise ValueError(f"snr_axis must be one of {list(SNR_AXES)}, got {snr_axis!r}")
    if spec.is_reference and snr_axis != "reference":
        raise ValueError(f"the reference channel has only its own SNR axis (snr_axis='reference'), got {snr_axis!r}")
    if not spec.is_reference and snr_axis == "reference":
        raise ValueError("snr_axis='reference' belongs to the reference channel: a channel model takes 'esn0' or 'ebn0'")
    return snr_axis


def sigmas_for_axis(spec, snr_axis, snrs, rate, speed=1.0, constellation=None):
    """sigma per SNR point under the axis (resolve_snr_axis has accepted it).
    constellation (a constellation.Constellation): the Eb/N0 axis uses the
    table's bits per symbol in place of the modulation's."""
    spec = spec or ChannelSpec()
    if constellation is not None and snr_axis == "ebn0":
        return [sigma_for_ebn0(s, rate, constellation.bps, table=True) for s in snrs]
    if snr_axis == "reference":
        return [1.0 / math.sqrt(2.0 * speed * (10.0 ** (s * 0.1))) for s in snrs]
    if snr_axis == "esn0":
        return [sigma_for_esn0(s) for s in snrs]
    return [sigma_for_ebn0(s, rate, spec.bps) for s in snrs]
