"""BER/FER Monte-Carlo sweep on the GPU(s) -- the caller of the hot path.

Reproduces the counter semantics of python_ldpc_app/main.py:run_simulation
(:178-442) with the frame pipeline on the device (ldpc_mc_run):
  * SNR grid: steps = ceil((end-start)/step) + 1, each point clamped to `end`
    (main.py:193, :206-209); sigma = 1/sqrt(2*speed*10^(snr/10)) (channel.py:113);
  * per frame: Result OK <=> syndrome zero; error bits counted only in frames
    whose decode FAILED (main.py:130-138); convergence iteration summed over
    converged frames (:154-172);
  * per point: FER = failed/B, BER = err/(k*B), avg_conv = sum/count,
    avg normalized LLR = sum/B (:346-369).
Multi-GPU (one process per GPU): rank r decodes the global frame indices
[r*B/W, (r+1)*B/W) of every SNR point -- the Philox stream is keyed by the
global index, so the counters are identical for any W -- and the whole
[points x 7] counter matrix is summed with ONE all-reduce: RCCL over xGMI
through the C ABI (ldpc_amd.comm, no PyTorch); the CPU tests inject a gloo
reducer of their own (tests/test_montecarlo.py) to exercise the same sharding
logic.
"""
import argparse
import math
import os
import time
from datetime import datetime

import numpy as np

from .results import SimulationConfig, SimulationResult, SNRPointResult

NCOUNT = 7  # frames, failed, err_bits, sum_conv, n_conv, sum_nllr_count, iters


def snr_grid(initial, end, step):
    """main.py:193,206-209."""
    steps = int(math.ceil((end - initial) / step)) + 1
    out = []
    for s in range(steps):
        v = initial + s * step
        out.append(end if v > end else v)
    return out


def sigma_for_snr(snr_db, speed=1.0):
    """channel.py:113 (mode 1)."""
    return 1.0 / math.sqrt(2.0 * speed * (10.0 ** (snr_db * 0.1)))


def shard(total, rank, world):
    """Balanced contiguous split of [0, total) -> (start, count) for `rank`."""
    base, extra = divmod(total, world)
    start = rank * base + min(rank, extra)
    return start, base + (1 if rank < extra else 0)


def point_results(counters, k, snrs, matrix_path="", max_iter=5):
    """Per-SNR SNRPointResult from the summed counter matrix (main.py:346-389)."""
    pts = []
    for snr, c in zip(snrs, counters):
        frames, failed, err, sconv, nconv, snllr = (int(x) for x in c[:6])
        pts.append(SNRPointResult(
            snr_db=float(snr),
            ber=(err / (k * frames)) if k * frames > 0 else 0.0,
            fer=failed / frames if frames else 0.0,
            avg_normalized_llr=(snllr / k) / frames if frames and k else 0.0,
            total_blocks=frames, successful_blocks=frames - failed, failed_blocks=failed,
            avg_convergence_iterations=(sconv / nconv) if nconv else 0.0,
            matrix_path=matrix_path, max_iterations=max_iter))
    return pts


def fer_by_max_iter(hist):
    """Detected FER for every iteration limit up to the run's, from one run's
    histogram (Decoder.mc_stats_read): float64 [T], entry T' - 1 =
    1 - sum_{t < T'} hist[t] / sum(hist), what a run with max_iter = T' over
    the same frames reports -- a physical decoder's first T' iterations do not
    depend on the limit.  All zeros for an empty histogram."""
    hist = np.asarray(hist, dtype=np.int64)
    T = len(hist) - 1
    total = int(hist.sum())
    if T < 1 or total == 0:
        return np.zeros(max(T, 0), np.float64)
    # (total - converged) / total in integers, one rounding: exactly the failed / frames of such a run
    return (total - np.cumsum(hist[:T])).astype(np.float64) / float(total)


def reduce_stats(stats, snrs, world=1, allreduce=None):
    """Per-point statistics of a sweep from this rank's Decoder.mc_stats_read
    dicts: with world > 1 the histograms and the undetected totals are summed
    over the ranks (int64, the counters' allreduce).  Failure lists are per
    rank and must be empty (max_failed = 0); failed_dropped is then every
    failed frame, hist[T] of the summed histogram.  Then snr_db, frames and
    fer_by_max_iter are added."""
    stats = [dict(st) for st in stats]
    if world > 1:
        if allreduce is None:
            raise ValueError("world > 1 needs an allreduce")
        if any(len(st["failed"]) for st in stats):
            raise ValueError("failed-frame lists are not gathered across ranks: max_failed must be 0 with world > 1")
        T1 = len(stats[0]["hist"])
        local = np.zeros((len(stats), T1 + 2), np.int64)
        for row, st in zip(local, stats):
            row[:T1] = st["hist"]
            row[T1:] = st["undetected_frames"], st["undetected_bit_errors"]
        total = np.asarray(allreduce(local), dtype=np.int64).reshape(local.shape)
        for row, st in zip(total, stats):
            st["hist"] = row[:T1].copy()
            st["undetected_frames"], st["undetected_bit_errors"] = int(row[T1]), int(row[T1 + 1])
            st["failed_dropped"] = int(row[T1 - 1])  # no records are kept: every failure of every rank
    for snr, st in zip(snrs, stats):
        st["hist"] = np.asarray(st["hist"], dtype=np.int64)
        st["snr_db"] = float(snr)
        st["frames"] = int(st["hist"].sum())
        st["fer_by_max_iter"] = fer_by_max_iter(st["hist"])
    return stats


def stats_to_json(path, seed, stats, channel=None):
    """Write the statistics of a sweep (reduce_stats) with its seed: the seed
    and a point's index and failed frame indices regenerate the failed frames
    (on a decoder with the same channel set).  channel: channel_info's dict of
    the sweep, written as the document's "channel" object."""
    import json
    pts = [{"snr_db": st["snr_db"], "frames": st["frames"], "hist": [int(x) for x in st["hist"]],
            "fer_by_max_iter": [float(x) for x in st["fer_by_max_iter"]],
            "undetected_frames": int(st["undetected_frames"]),
            "undetected_bit_errors": int(st["undetected_bit_errors"]),
            "failed": [[int(i), int(e)] for i, e in np.asarray(st["failed"]).reshape(-1, 2)],
            "failed_dropped": int(st["failed_dropped"])} for st in stats]
    with open(path, "w") as f:
        doc = {"seed": int(seed), "points": pts}
        if channel is not None:
            doc["channel"] = channel
        json.dump(doc, f, indent=1)


def run_sweep(decoder, snrs, blocks, max_iter, seed=20260213, nllr=False, speed=1.0,
              rank=0, world=1, allreduce=None, counter_fn=None, stats_fn=None, sigmas=None):
    """Counters [len(snrs), 7] for `blocks` frames per SNR point, summed over ranks.

    decoder     ldpc_amd.device.Decoder (its graph fixes the code) -- or None with counter_fn
    counter_fn  (sigmas, count, frame0) -> int64 [points, 7]; defaults to
                decoder.mc_run (the GPU path).  Tests inject a CPU stand-in to
                exercise the sharding/all-reduce logic without a GPU.
    allreduce   callable(np.ndarray int64) -> summed array (ldpc_amd.comm.Comm.allreduce)
    stats_fn    point index -> Decoder.mc_stats_read dict of the run counter_fn
                just made; given, the result is (counters, reduce_stats(...))
    sigmas      sigma per SNR point where the axis is not the reference's
                (channel.sigmas_for_axis); default sigma_for_snr
    """
    sig = [sigma_for_snr(s, speed) for s in snrs] if sigmas is None else [float(x) for x in sigmas]
    if len(sig) != len(snrs):
        raise ValueError(f"sigmas has {len(sig)} entries for {len(snrs)} SNR points")
    start, count = shard(int(blocks), rank, world)
    if counter_fn is None:
        def counter_fn(sigmas, cnt, frame0):
            return decoder.mc_run(seed, sigmas, cnt, frame0, max_iter, nllr=nllr)
    local = np.asarray(counter_fn(sig, count, start), dtype=np.int64).reshape(len(snrs), NCOUNT)
    if world > 1:
        if allreduce is None:
            raise ValueError("world > 1 needs an allreduce")
        local = np.asarray(allreduce(local), dtype=np.int64).reshape(len(snrs), NCOUNT)
    if stats_fn is not None:
        return local, reduce_stats([stats_fn(p) for p in range(len(snrs))], snrs, world, allreduce)
    return local


# Codes built in code, not loaded: IRA graphs H = [H_info | staircase] (ldpc_amd.ira),
# physical mode only -- the graph is its own frame source (parities by accumulation),
# and its H_std = [A | I] would be dense.
IRA_CODES = {"dvbs2_profile_64800_0.5": "dvbs2_profile_matrix", "ira_1440_0.5": "small_ira_matrix"}


def check_ira_mode(matrix, mode):
    """ValueError for an IRA code name outside physical mode."""
    if isinstance(matrix, str) and matrix in IRA_CODES and mode != "physical":
        raise ValueError(f"{matrix} is an IRA code decoded on its sparse graph: it needs mode='physical' "
                         "(its H_std = [A | I] is dense; parity mode has no decoder for it)")


DECODER_TYPES = {"spa": "sumproduct", "nms": "minsum-normalized", "oms": "minsum-offset"}


def decoder_type(cn_rule="spa", schedule="flooding", qbits=None):
    """The result schema's decoder_type for a check rule, a schedule and (fixed
    point) the message width, e.g. "minsum-normalized-layered-q6"."""
    return (DECODER_TYPES[cn_rule] + ("-layered" if schedule == "layered" else "")
            + (f"-q{int(qbits)}" if qbits is not None else ""))


DECODERS = ("sumproduct", "bitflipping")  # the reference's --decoder values


def bitflip_decoder_type(weight=0.0):
    """The result schema's decoder_type of a bit-flipping sweep: "bitflipping"
    for weight == 0 (hard decisions only), else "bitflipping-gd"."""
    return "bitflipping" if float(weight) == 0.0 else "bitflipping-gd"


def check_decoder_args(decoder, bf_weight, bf_theta, mode, cn_rule="spa", schedule="flooding", qbits=None,
                       layered_tile=False, quant_tile=False, nllr=False):
    """ValueError for a decoder choice simulate() cannot honour (before any
    device call): "bitflipping" needs mode="physical" and none of the
    message-passing options; bf_weight / bf_theta need "bitflipping".  Returns
    (weight, theta) as device.bitflip_args does."""
    from .device import bitflip_args
    if decoder not in DECODERS:
        raise ValueError(f"decoder must be one of {DECODERS}, got {decoder!r}")
    weight, theta = bitflip_args(bf_weight, bf_theta)
    if decoder != "bitflipping":
        if weight != 0.0 or theta != 0.0:
            raise ValueError("bf_weight / bf_theta need decoder='bitflipping'")
        return weight, theta
    if mode != "physical":
        raise ValueError("decoder='bitflipping' needs mode='physical' (parity mode is the reference's sum-product)")
    if (cn_rule, schedule) != ("spa", "flooding") or qbits is not None or layered_tile or quant_tile or nllr:
        raise ValueError("decoder='bitflipping' passes no messages: cn_rule, schedule, qbits, layered_tile, "
                         "quant_tile and nllr do not apply to it")
    return weight, theta


def simulate(matrix, snrs, blocks, max_iter, seed=20260213, nllr=False, chunk=65536, device=0,
             rank=0, world=1, allreduce=None, matrix_path="", mode="parity", cn_rule="spa", schedule="flooding",
             alpha=0.75, beta=0.5, qbits=None, llr_scale=4.0, layered_tile=False, quant_tile=False, stats=False,
             max_failed=0, channel=None, snr_axis=None, rate_match=None, decoder="sumproduct", bf_weight=0.0,
             bf_theta=0.0, interleaver=None, fading_block=1, constellation=None):
    """Full sweep on this process's GPU -> SimulationResult (reference schema).

    mode "parity" is the reference's decoder on H_std; "physical" decodes the
    same on-device frames on the sparse graph (Decoder.phys_mc_run) with the
    check rule cn_rule ("spa", "nms", "oms"; alpha / beta) and the schedule
    ("flooding", "layered") -- those options need mode="physical".  qbits
    (4..8) selects the fixed-point min-sum decoder on LLRs scaled by llr_scale
    (device.phys_quant_args); it needs mode="physical" and a min-sum rule.
    layered_tile runs the layered schedule on the HBM tile kernels even where
    the state fits LDS (it needs schedule="layered"; a code too large for LDS
    takes them anyway); quant_tile does the same for the fixed-point decoder
    (it needs qbits; either schedule).  matrix may name an IRA code (IRA_CODES): physical
    mode only, the graph itself is the frame source.
    stats=True (physical mode) also collects the Monte-Carlo statistics and
    returns (result, counters, stats): per point the Decoder.mc_stats_read dict
    (up to max_failed failed-frame records) plus snr_db, frames and
    fer_by_max_iter; with world > 1 the histograms and undetected totals are
    summed over the ranks and max_failed must be 0.
    channel (a channel.ChannelSpec; None = the reference channel) puts a
    textbook channel model under the frames; it needs mode="physical".
    snr_axis says what `snrs` are: "reference" (the reference channel's own
    axis, and the only one it has), "esn0" or "ebn0" (the models; Eb/N0 with the
    code's k/n and the modulation's bits per symbol); None = "reference" for
    the reference channel, "ebn0" for a model.
    rate_match (a ratematch.RateMatch; None = every column is sent) punctures
    and shortens the frames; it needs mode="physical" and a channel model.  The
    Eb/N0 axis and the config's rate then use the effective rate
    (k - n_short) / E, the BER counts k - n_short information bits, and the
    config's n, m, k stay the mother code's.
    decoder "bitflipping" (physical mode; the reference's --decoder value, which
    it never dispatches) decodes the same frames by bit flipping with
    bf_weight / bf_theta (device.bitflip_decode; Decoder.bitflip_mc_run); the
    message-passing options must be at their defaults.  stats, channel,
    snr_axis, rate_match and rank / world work as for the other decoders.
    interleaver (an interleave.Interleaver, or one of its spec strings: none,
    regular, block:R, random[:seed], srandom:S[:seed], file:PATH; None = the
    frame's column order) permutes the transmitted bits before they are mapped
    to symbols; a spec is resolved against E once the code and the pattern are
    known.  It needs mode="physical" and a channel model.  fading_block (an
    integer >= 1, or "frame") is the Rayleigh channel's coherence length in
    symbols (BPSK: bits): 1 is a fade per symbol, "frame" one fade per frame;
    anything but 1 needs channel model "rayleigh".
    constellation (a constellation.Constellation; None = the channel's own
    modulation) replaces the modulation by a table of 2^bps complex points: the
    Eb/N0 axis and every divisibility check then use the table's bits per
    symbol.  It needs mode="physical" and channel model "awgn" or "rayleigh"."""
    bf_weight, bf_theta = check_decoder_args(decoder, bf_weight, bf_theta, mode, cn_rule, schedule, qbits,
                                             layered_tile, quant_tile, nllr)
    bf = (bf_weight, bf_theta) if decoder == "bitflipping" else None
    check_constellation_args(constellation, channel, mode)
    snr_axis = check_channel_args(channel, snr_axis, mode)
    rate_match = check_rate_match_args(rate_match, channel, mode)
    interleaver, fading_block = check_interleave_args(interleaver, fading_block, channel, mode)
    from .channel import sigmas_for_axis
    from .code import EncoderDecoderData, load_committed_code
    from .device import Decoder, Graph, phys_flags, phys_quant_args, phys_rule_args
    if mode not in ("parity", "physical"):
        raise ValueError(f"mode must be 'parity' or 'physical', got {mode!r}")
    check_stats_args(stats, max_failed, mode, world)
    phys_rule_args(cn_rule, schedule, alpha, beta)  # ValueError before any device call
    if mode == "parity" and (cn_rule, schedule) != ("spa", "flooding"):
        raise ValueError("cn_rule / schedule need mode='physical' (parity mode is the reference's sum-product)")
    if qbits is not None:
        if mode != "physical":
            raise ValueError("qbits needs mode='physical'")
        phys_quant_args(cn_rule, alpha, beta, qbits, llr_scale)
    elif quant_tile:
        raise ValueError("quant_tile needs qbits (the fixed-point decoder)")
    phys_flags(tile=layered_tile, schedule=schedule, qtile=quant_tile)
    check_ira_mode(matrix, mode)
    t0 = time.time()
    if isinstance(matrix, str) and matrix in IRA_CODES:
        from . import ira
        return _simulate_graph(getattr(ira, IRA_CODES[matrix])(), matrix, t0, snrs, blocks, max_iter, seed, chunk,
                               device, rank, world, allreduce, matrix_path, cn_rule, schedule, alpha, beta, qbits,
                               llr_scale, layered_tile, quant_tile, stats, max_failed, channel, snr_axis, rate_match,
                               bf, interleaver, fading_block, constellation)
    if isinstance(matrix, EncoderDecoderData):
        edd = matrix
    elif isinstance(matrix, str) and os.path.exists(matrix):
        edd = EncoderDecoderData(matrix)
    else:
        edd = load_committed_code(matrix)
    sigmas = None
    rate, k_info = edd._rate, edd._k
    if channel is not None and not channel.is_reference:
        # ValueErrors before any device call
        sent, k_info, rate = rate_match_shape(rate_match, channel, edd._n, edd._k, constellation)
        (constellation or channel).check_length(sent)
        interleaver = resolve_interleaver(interleaver, sent)
        sigmas = sigmas_for_axis(channel, snr_axis, snrs, rate, constellation=constellation)
    g = Graph(edd._h_std, device=device)
    dec = Decoder(g, Decoder.fit_slots(g, min(max(1, shard(int(blocks), rank, world)[1]), chunk)))
    if sigmas is not None:
        dec.set_channel(channel)
        dec.set_rate_match(rate_match)
        dec.set_interleaver(interleaver)
        dec.set_fading_block(fading_block)
        dec.set_constellation(constellation)
    counter_fn = None
    if stats:
        dec.mc_stats(True, max_failed)
    if mode == "physical":
        gp = Graph(edd.physical_matrix(), device=device)

        def counter_fn(sigmas, cnt, frame0):
            if bf is not None:
                return dec.bitflip_mc_run(gp, seed, sigmas, cnt, frame0, max_iter, weight=bf[0], theta=bf[1])
            return dec.phys_mc_run(gp, seed, sigmas, cnt, frame0, max_iter, cn=cn_rule, schedule=schedule,
                                   alpha=alpha, beta=beta, qbits=qbits, llr_scale=llr_scale, tile=layered_tile,
                                   qtile=quant_tile)
    ctr = run_sweep(dec, snrs, blocks, max_iter, seed=seed, nllr=nllr, rank=rank, world=world,
                    allreduce=allreduce, counter_fn=counter_fn,
                    stats_fn=(lambda p: dec.mc_stats_read(p, max_iter)) if stats else None, sigmas=sigmas)
    ctr, st = ctr if stats else (ctr, None)
    pts = point_results(ctr, k_info, snrs, matrix_path=matrix_path or str(matrix), max_iter=max_iter)
    cfg = SimulationConfig(
        matrix_path=matrix_path or str(matrix), n=edd._n, m=edd._m, k=edd._k, rate=rate,
        blocks=int(blocks), max_iterations=int(max_iter), encoding_method="standard",
        interleaver_type=interleaver.kind if interleaver is not None else "none",
        decoder_type=bitflip_decoder_type(bf[0]) if bf is not None else decoder_type(cn_rule, schedule, qbits),
        channel_mode=1, modulation=1,
        speed=1.0, snr_range=(snrs[0], snrs[-1], (snrs[1] - snrs[0]) if len(snrs) > 1 else 0.0),
        threads=world, timestamp=datetime.now().isoformat())
    res = SimulationResult(config=cfg, snr_points=pts, wall_clock_seconds=time.time() - t0)
    return (res, ctr, st) if stats else (res, ctr)


def check_channel_args(channel, snr_axis, mode):
    """ValueError for a channel / SNR axis simulate() cannot honour (before any
    code is loaded); returns the axis in force (channel.resolve_snr_axis)."""
    from .channel import ChannelSpec, resolve_snr_axis
    if channel is not None and not isinstance(channel, ChannelSpec):
        raise ValueError(f"channel must be a ChannelSpec or None, got {type(channel).__name__}")
    if channel is not None and not channel.is_reference and mode != "physical":
        raise ValueError(f"the {channel.model} channel needs mode='physical' (the channel models are physical "
                         "mode's; parity mode reproduces the reference's channel)")
    return resolve_snr_axis(channel, snr_axis)


def check_constellation_args(constellation, channel, mode):
    """ValueError for a constellation table simulate() cannot honour (before any
    code is loaded): it replaces the modulation of a channel model."""
    from .constellation import Constellation
    if constellation is None:
        return None
    if not isinstance(constellation, Constellation):
        raise ValueError(f"constellation must be a Constellation or None, got {type(constellation).__name__}")
    if mode != "physical":
        raise ValueError("constellation needs mode='physical' (parity mode reproduces the reference's BPSK channel)")
    if channel is None or channel.is_reference:
        raise ValueError("constellation needs a channel model (channel=ChannelSpec('awgn' / 'rayleigh', ...)): the "
                         "reference channel is BPSK only")
    return constellation


def check_rate_match_args(rate_match, channel, mode):
    """ValueError for a rate-matching pattern simulate() cannot honour (before
    any code is loaded); returns the pattern, None for an empty one."""
    from .ratematch import RateMatch
    if rate_match is None:
        return None
    if not isinstance(rate_match, RateMatch):
        raise ValueError(f"rate_match must be a RateMatch or None, got {type(rate_match).__name__}")
    if rate_match.is_empty:
        return None
    if mode != "physical":
        raise ValueError("rate_match needs mode='physical' (parity mode sends every code whole)")
    if channel is None or channel.is_reference:
        raise ValueError("rate_match needs a channel model (channel=ChannelSpec('awgn' / 'rayleigh', ...)): the "
                         "reference channel sends every code whole")
    return rate_match


FADING_FRAME = 2 ** 31 - 1  # fading_block="frame": a coherence length no frame reaches


def check_interleave_args(interleaver, fading_block, channel, mode):
    """ValueError for an interleaver / coherence length simulate() cannot
    honour (before any code is loaded); returns (interleaver, fading_block)
    with "none" as None and "frame" as FADING_FRAME.  A spec string is checked
    for its form here and resolved once E is known (resolve_interleaver)."""
    from .interleave import Interleaver, split_spec
    model = channel is not None and not channel.is_reference
    if isinstance(interleaver, str):
        if split_spec(interleaver)[0] == "none":
            interleaver = None
    elif interleaver is not None and not isinstance(interleaver, Interleaver):
        raise ValueError(f"interleaver must be an Interleaver, a spec string or None, got {type(interleaver).__name__}")
    if interleaver is not None:
        if mode != "physical":
            raise ValueError("interleaver needs mode='physical' (parity mode sends every code in column order)")
        if not model:
            raise ValueError("interleaver needs a channel model (channel=ChannelSpec('awgn' / 'rayleigh', ...)): it "
                             "cannot change decoding on the memoryless reference channel")
    if isinstance(fading_block, str):
        if fading_block.strip().lower() != "frame":
            raise ValueError(f"fading_block must be an integer >= 1 or 'frame', got {fading_block!r}")
        fading_block = FADING_FRAME
    if isinstance(fading_block, bool) or not isinstance(fading_block, int) or not 1 <= fading_block <= FADING_FRAME:
        raise ValueError(f"fading_block must be an integer in [1, {FADING_FRAME}] or 'frame', got {fading_block!r}")
    if fading_block > 1:
        if mode != "physical":
            raise ValueError("fading_block needs mode='physical'")
        if not model or channel.model != "rayleigh":
            raise ValueError("fading_block > 1 needs the Rayleigh channel (channel=ChannelSpec('rayleigh', ...)): "
                             "no other model has a fade")
    return interleaver, fading_block


def resolve_interleaver(interleaver, E):
    """The Interleaver of simulate()'s argument for E transmitted bits (None
    without one); ValueError where the spec or the length does not fit."""
    from .interleave import resolve
    return resolve(interleaver, E)


def interleave_header(info):
    """The command line's header line of an interleaved / block-faded sweep."""
    il = info.get("interleaver")
    what = "none" if il is None else " ".join(f"{k} {v}" for k, v in il.items())
    fb = info.get("fading_block", 1)
    return f"interleaver {what}  coherence length {fb}" + ("" if fb == "frame" else " symbol(s)")


def rate_match_shape(rate_match, channel, n, k, constellation=None):
    """(transmitted bits E, information bits, effective rate) of an (n, k) code
    under the pattern (None: n, k, k / n); ValueError for a pattern the code or
    the bits per symbol (the constellation table's, else the channel's) cannot
    carry."""
    from .constellation import effective_bps
    if rate_match is None or rate_match.is_empty:
        return int(n), int(k), k / n
    rate_match.validate(n, k, effective_bps(channel, constellation))
    return rate_match.n_transmitted(n), rate_match.info_bits(k), rate_match.effective_rate(n, k)


def channel_info(channel, snr_axis, snrs, rate, rate_match=None, n=None, k=None, interleaver=None, fading_block=1,
                 constellation=None):
    """The sweep's channel as --stats-json writes it: model, modulation, demap,
    snr_axis and sigma per point; under a rate-matching pattern (then with the
    mother code's n and k, and `rate` the effective rate) also "rate_match":
    the columns, the transmitted and information bits and the rate; with an
    interleaver (an Interleaver) "interleaver": its info(); with a coherence
    length other than 1 "fading_block" (FADING_FRAME as "frame"); under a
    constellation table "constellation": its name, bps and points (sigma then
    follows the table's bps, and "modulation" is what the table replaced)."""
    from .channel import ChannelSpec, resolve_snr_axis, sigmas_for_axis
    channel = channel or ChannelSpec()
    snr_axis = resolve_snr_axis(channel, snr_axis)
    info = {"model": channel.model, "modulation": channel.modulation, "demap": channel.demap, "snr_axis": snr_axis,
            "sigma": [float(x) for x in sigmas_for_axis(channel, snr_axis, snrs, rate, constellation=constellation)]}
    if constellation is not None:
        info["constellation"] = constellation.info()
    if rate_match is not None and not rate_match.is_empty:
        info["rate_match"] = rate_match.info(n, k)
    if interleaver is not None:
        info["interleaver"] = interleaver.info()
    if fading_block != 1:
        info["fading_block"] = "frame" if fading_block == FADING_FRAME else int(fading_block)
    return info


def check_stats_args(stats, max_failed, mode, world):
    """ValueError for statistics options simulate() cannot honour (before any device call)."""
    if int(max_failed) < 0:
        raise ValueError(f"max_failed must be >= 0, got {max_failed}")
    if max_failed and not stats:
        raise ValueError("max_failed needs stats=True")
    if stats and mode != "physical":
        raise ValueError("stats needs mode='physical' (parity mode collects no Monte-Carlo statistics)")
    if stats and world > 1 and max_failed > 0:
        raise ValueError("max_failed > 0 needs world == 1: failed-frame lists are not gathered across ranks")


def _simulate_graph(H, name, t0, snrs, blocks, max_iter, seed, chunk, device, rank, world, allreduce, matrix_path,
                    cn_rule, schedule, alpha, beta, qbits, llr_scale, layered_tile, quant_tile=False, stats=False,
                    max_failed=0, channel=None, snr_axis="reference", rate_match=None, bf=None, interleaver=None,
                    fading_block=1, constellation=None):
    """simulate() in physical mode on an IRA graph H: one graph, the decoder's
    frame source and the graph it decodes on (as bench.py's config 5).
    bf: (weight, theta) of the bit-flipping decoder, None for the others."""
    from .device import Decoder, Graph
    m, n = H.shape
    k = n - m
    sigmas = None
    rate, k_info = k / n, k
    if channel is not None and not channel.is_reference:
        from .channel import sigmas_for_axis
        # ValueErrors before any device call
        sent, k_info, rate = rate_match_shape(rate_match, channel, n, k, constellation)
        (constellation or channel).check_length(sent)
        interleaver = resolve_interleaver(interleaver, sent)
        sigmas = sigmas_for_axis(channel, snr_axis, snrs, rate, constellation=constellation)
    g = Graph(H, device=device)
    dec = Decoder(g, Decoder.fit_slots(g, min(max(1, shard(int(blocks), rank, world)[1]), chunk)))
    if sigmas is not None:
        dec.set_channel(channel)
        dec.set_rate_match(rate_match)
        dec.set_interleaver(interleaver)
        dec.set_fading_block(fading_block)
        dec.set_constellation(constellation)

    def counter_fn(sigmas, cnt, frame0):
        if bf is not None:
            return dec.bitflip_mc_run(g, seed, sigmas, cnt, frame0, max_iter, weight=bf[0], theta=bf[1])
        return dec.phys_mc_run(g, seed, sigmas, cnt, frame0, max_iter, cn=cn_rule, schedule=schedule, alpha=alpha,
                               beta=beta, qbits=qbits, llr_scale=llr_scale, tile=layered_tile, qtile=quant_tile)
    if stats:
        dec.mc_stats(True, max_failed)
    ctr = run_sweep(dec, snrs, blocks, max_iter, seed=seed, rank=rank, world=world, allreduce=allreduce,
                    counter_fn=counter_fn, stats_fn=(lambda p: dec.mc_stats_read(p, max_iter)) if stats else None,
                    sigmas=sigmas)
    ctr, st = ctr if stats else (ctr, None)
    pts = point_results(ctr, k_info, snrs, matrix_path=matrix_path or name, max_iter=max_iter)
    cfg = SimulationConfig(
        matrix_path=matrix_path or name, n=n, m=m, k=k, rate=rate, blocks=int(blocks),
        max_iterations=int(max_iter), encoding_method="standard",
        interleaver_type=interleaver.kind if interleaver is not None else "none",
        decoder_type=bitflip_decoder_type(bf[0]) if bf is not None else decoder_type(cn_rule, schedule, qbits),
        channel_mode=1, modulation=1, speed=1.0,
        snr_range=(snrs[0], snrs[-1], (snrs[1] - snrs[0]) if len(snrs) > 1 else 0.0), threads=world,
        timestamp=datetime.now().isoformat())
    res = SimulationResult(config=cfg, snr_points=pts, wall_clock_seconds=time.time() - t0)
    return (res, ctr, st) if stats else (res, ctr)


def check_harq_args(harq, channel, mode, interleaver=None, rate_match=None):
    """ValueError for a HARQ plan simulate_harq() cannot honour (before any
    code is loaded): it needs mode="physical" and a channel model, and neither
    an interleaver nor punctured columns (the plan says what is sent, in which
    order).  A spec string is checked for its form here and resolved once the
    code is known (harq.resolve)."""
    from .harq import HarqPlan, split_spec
    if isinstance(harq, str):
        split_spec(harq)
    elif not isinstance(harq, HarqPlan):
        raise ValueError(f"harq must be a HarqPlan or a spec string, got {type(harq).__name__}")
    if mode != "physical":
        raise ValueError("a HARQ plan needs mode='physical' (parity mode sends every code once)")
    if channel is None or channel.is_reference:
        raise ValueError("a HARQ plan needs a channel model (channel=ChannelSpec('awgn' / 'rayleigh', ...)): the "
                         "reference channel sends every code once")
    if interleaver is not None and not (isinstance(interleaver, str) and interleaver.strip().lower() == "none"):
        raise ValueError("a HARQ plan carries its own order on the air: it takes no interleaver")
    if rate_match is not None and rate_match.punctured:
        raise ValueError("a HARQ plan says what is sent: it takes no puncturing pattern (shortening may stay)")
    return harq


def harq_point(counters, lengths, k_info, bps):
    """The HARQ figures of one SNR point from the counters of the R sweeps,
    counters[r] being the run with the first r + 1 transmissions (int64 [R, 7]
    in NCOUNT's order) and lengths[r] = E_r:
      fer_after[r]      failed / frames of run r
      ber_after[r]      err_bits / (k_info frames)
      avg_iterations[r] iterations / frames
      p_tx[r]           the probability that transmission r is sent: 1 for
                        r = 0, fer_after[r - 1] after
      avg_tx            sum p_tx
      bits_sent         sum p_tx[r] E_r
      throughput        k_info (1 - fer_after[R - 1]) / (bits_sent / bps),
                        information bits per symbol
    p_tx treats the failures as nested: it is exact where a frame that decodes
    from r transmissions also decodes from more, which combining makes very
    nearly but not strictly so."""
    c = np.asarray(counters, dtype=np.int64).reshape(-1, NCOUNT)
    R = c.shape[0]
    if len(lengths) != R:
        raise ValueError(f"{len(lengths)} transmission lengths for {R} runs")
    frames = c[:, 0].astype(np.float64)
    ok = frames > 0
    safe = np.where(ok, frames, 1.0)
    fer = np.where(ok, c[:, 1] / safe, 0.0)
    ber = np.where(ok, c[:, 2] / (float(k_info) * safe), 0.0) if k_info else np.zeros(R)
    avg_it = np.where(ok, c[:, 6] / safe, 0.0)
    p_tx = np.concatenate([[1.0], fer[:-1]])
    bits = float(np.sum(p_tx * np.asarray(lengths, dtype=np.float64)))
    return {"fer_after": [float(x) for x in fer], "ber_after": [float(x) for x in ber],
            "avg_iterations": [float(x) for x in avg_it], "p_tx": [float(x) for x in p_tx],
            "avg_tx": float(p_tx.sum()), "bits_sent": bits,
            "throughput": float(k_info) * (1.0 - float(fer[-1])) / (bits / float(bps))}


def simulate_harq(matrix, snrs, blocks, max_iter, harq, seed=20260213, chunk=65536, device=0, rank=0, world=1,
                  allreduce=None, mode="physical", cn_rule="spa", schedule="flooding", alpha=0.75, beta=0.5,
                  qbits=None, llr_scale=4.0, layered_tile=False, quant_tile=False, stats=False, max_failed=0,
                  channel=None, snr_axis=None, rate_match=None, decoder="sumproduct", bf_weight=0.0, bf_theta=0.0,
                  interleaver=None, fading_block=1, constellation=None):
    """A physical-mode sweep under a HARQ plan (harq: a harq.HarqPlan, or one of
    its spec strings chase:R[:E], ir:R:E, file:PATH, resolved against the code
    and the pattern's shortened columns).  The keywords are simulate()'s
    physical-mode ones.  The sweep runs R times on the same seed, run r with the
    plan's first r + 1 transmissions (HarqPlan.truncated), so run r decodes
    exactly the frames a receiver holds after transmission r, each regenerable
    from (seed, point, frame index).  Returns a dict:
      "plan"      HarqPlan.info()
      "sigma"     sigma per point (the same for every transmission)
      "counters"  int64 [R, points, 7]
      "points"    per SNR point snr_db, frames and harq_point()'s figures:
                  fer_after, ber_after, avg_iterations, p_tx, avg_tx, bits_sent,
                  throughput
      "stats"     stats=True: per run the per-point statistics of simulate()
    p_tx treats the failures as nested (harq_point), which is exact where a
    frame that decodes from r transmissions also decodes from more.  An Eb/N0
    axis uses the first transmission's rate (k - n_short) / E_0.
    ValueError before any device call for a plan without a channel model, with
    an interleaver, with a puncturing pattern, or in parity mode."""
    bf_weight, bf_theta = check_decoder_args(decoder, bf_weight, bf_theta, mode, cn_rule, schedule, qbits,
                                             layered_tile, quant_tile, False)
    bf = (bf_weight, bf_theta) if decoder == "bitflipping" else None
    check_harq_args(harq, channel, mode, interleaver, rate_match)
    check_constellation_args(constellation, channel, mode)
    snr_axis = check_channel_args(channel, snr_axis, mode)
    rate_match = check_rate_match_args(rate_match, channel, mode)
    _, fading_block = check_interleave_args(None, fading_block, channel, mode)
    from .channel import sigmas_for_axis
    from .code import EncoderDecoderData, load_committed_code
    from .device import Decoder, Graph, phys_flags, phys_quant_args, phys_rule_args
    from .constellation import effective_bps
    from .harq import resolve as resolve_harq
    check_stats_args(stats, max_failed, mode, world)
    phys_rule_args(cn_rule, schedule, alpha, beta)
    if qbits is not None:
        phys_quant_args(cn_rule, alpha, beta, qbits, llr_scale)
    elif quant_tile:
        raise ValueError("quant_tile needs qbits (the fixed-point decoder)")
    phys_flags(tile=layered_tile, schedule=schedule, qtile=quant_tile)
    if isinstance(matrix, str) and matrix in IRA_CODES:
        from . import ira
        H = getattr(ira, IRA_CODES[matrix])()
        m, n = H.shape
        k = n - m
        h_src = h_phys = H
    else:
        if isinstance(matrix, EncoderDecoderData):
            edd = matrix
        elif isinstance(matrix, str) and os.path.exists(matrix):
            edd = EncoderDecoderData(matrix)
        else:
            edd = load_committed_code(matrix)
        n, k = edd._n, edd._k
        h_src, h_phys = edd._h_std, None
    shortened = rate_match.shortened if rate_match is not None else ()
    if rate_match is not None:
        rate_match.validate(n, k)
    bps = effective_bps(channel, constellation)
    plan = resolve_harq(harq, n, shortened).validate(n, shortened, bps)
    k_info = k - len(shortened)
    sigmas = sigmas_for_axis(channel, snr_axis, snrs, k_info / plan.n_sent(0), constellation=constellation)
    g = Graph(h_src, device=device)
    gp = g if h_phys is h_src else Graph(edd.physical_matrix(), device=device)
    dec = Decoder(g, Decoder.fit_slots(g, min(max(1, shard(int(blocks), rank, world)[1]), chunk)))
    dec.set_channel(channel)
    dec.set_rate_match(rate_match)
    dec.set_fading_block(fading_block)
    dec.set_constellation(constellation)
    if stats:
        dec.mc_stats(True, max_failed)

    def counter_fn(sigmas, cnt, frame0):
        if bf is not None:
            return dec.bitflip_mc_run(gp, seed, sigmas, cnt, frame0, max_iter, weight=bf[0], theta=bf[1])
        return dec.phys_mc_run(gp, seed, sigmas, cnt, frame0, max_iter, cn=cn_rule, schedule=schedule, alpha=alpha,
                               beta=beta, qbits=qbits, llr_scale=llr_scale, tile=layered_tile, qtile=quant_tile)
    ctrs, sts = [], []
    for r in range(1, plan.R + 1):
        dec.set_harq(plan.truncated(r))
        out = run_sweep(dec, snrs, blocks, max_iter, seed=seed, rank=rank, world=world, allreduce=allreduce,
                        counter_fn=counter_fn, stats_fn=(lambda p: dec.mc_stats_read(p, max_iter)) if stats else None,
                        sigmas=sigmas)
        ctr, st = out if stats else (out, None)
        ctrs.append(np.asarray(ctr, dtype=np.int64))
        sts.append(st)
    ctrs = np.stack(ctrs)
    pts = []
    for p, snr in enumerate(snrs):
        pts.append({"snr_db": float(snr), "frames": int(ctrs[0, p, 0]),
                    **harq_point(ctrs[:, p], plan.lengths, k_info, bps)})
    res = {"plan": plan.info(), "sigma": [float(x) for x in sigmas], "counters": ctrs, "points": pts}
    if constellation is not None:
        res["constellation"] = constellation.info()
    if stats:
        res["stats"] = sts
    return res


def harq_header(info):
    """The command line's header line of a HARQ sweep."""
    step = f"  step {info['step']}" if "step" in info else ""
    return f"HARQ {info['kind']}  R {info['R']}  E_r " + " ".join(str(e) for e in info["E"]) + step


def harq_to_json(path, seed, res):
    """Write simulate_harq()'s result (without the statistics) with its seed."""
    import json
    doc = {"seed": int(seed), "plan": res["plan"], "sigma": res["sigma"], "points": res["points"],
           "counters": np.asarray(res["counters"]).tolist()}
    if "constellation" in res:
        doc["constellation"] = res["constellation"]
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)


def build_parser():
    ap = argparse.ArgumentParser(description="GPU BER/FER sweep (main.py semantics, AWGN mode 1, BPSK)")
    ap.add_argument("--matrix", required=True,
                    help="ALIST path, a committed code name, or (physical mode) " + " / ".join(sorted(IRA_CODES)))
    ap.add_argument("-b", "--blocks", type=int, default=1000)
    ap.add_argument("-i", "--iterations", type=int, default=5)
    ap.add_argument("--initial-snr", type=float, default=0.0)
    ap.add_argument("--end-snr", type=float, default=3.0)
    ap.add_argument("--step-snr", type=float, default=1.0)
    ap.add_argument("--normalized-llr", action="store_true")
    ap.add_argument("--seed", type=int, default=20260213)
    ap.add_argument("--output-json")
    ap.add_argument("--output-csv")
    ap.add_argument("--mode", choices=("parity", "physical"), default="parity",
                    help="parity: the reference's decoder on H_std; physical: the sparse graph, fp32")
    ap.add_argument("--cn-rule", choices=("spa", "nms", "oms"), default="spa",
                    help="physical mode: sum-product, normalized or offset min-sum")
    ap.add_argument("--schedule", choices=("flooding", "layered"), default="flooding",
                    help="physical mode: layered needs a min-sum rule")
    ap.add_argument("--layered-tile", action="store_true",
                    help="physical mode, --schedule layered: the HBM tile kernels even where the state fits LDS")
    ap.add_argument("--alpha", type=float, default=None, help="normalized min-sum factor in (0, 1] (default 0.75)")
    ap.add_argument("--beta", type=float, default=None, help="offset min-sum offset >= 0 (default 0.5)")
    ap.add_argument("--qbits", type=int, default=None,
                    help="physical mode, min-sum rules: fixed-point decoder with messages of 4..8 bits")
    ap.add_argument("--llr-scale", type=float, default=None,
                    help="with --qbits: quantizer steps per unit of LLR (default 4)")
    ap.add_argument("--quant-tile", action="store_true",
                    help="with --qbits: the HBM tile kernels even where the quantized state fits LDS")
    ap.add_argument("--decoder", choices=DECODERS, default="sumproduct",
                    help="the reference's flag: bitflipping (physical mode) is parallel gradient-descent bit flipping, "
                         "the hard-decision baseline")
    ap.add_argument("--bf-weight", type=float, default=None,
                    help="with --decoder bitflipping: weight of the channel term, >= 0 (default 0: hard decisions only)")
    ap.add_argument("--bf-theta", type=float, default=None,
                    help="with --decoder bitflipping: flip where the inversion function is below this (default 0)")
    ap.add_argument("--stats-json", default=None, metavar="PATH",
                    help="physical mode: write the per-point Monte-Carlo statistics (convergence histogram, "
                         "FER by iteration limit, undetected errors, failed frames) to PATH")
    ap.add_argument("--max-failed", type=int, default=0, metavar="N",
                    help="with --stats-json: keep up to N failed-frame records per SNR point (default 0)")
    ap.add_argument("--channel", choices=("reference", "awgn", "rayleigh"), default="reference",
                    help="physical mode: a textbook channel model under the frames (default: the reference's channel)")
    ap.add_argument("--modulation", choices=("bpsk", "qpsk", "qam16", "qam64"), default=None,
                    help="with --channel awgn / rayleigh: Gray-mapped square constellation (default bpsk)")
    ap.add_argument("--constellation", default=None, metavar="SPEC",
                    help="with --channel awgn / rayleigh, in place of --modulation: a table of 2^bps complex points, "
                         "demapped over all of them: 8psk, 16apsk[:GAMMA] (ring ratio, default 3.15; both labellings "
                         "are this project's own, see ldpc_amd/constellation.py) or file:PATH (one `re im` per line, "
                         "the line index is the label, unit mean energy)")
    ap.add_argument("--demap", choices=("exact", "maxlog"), default="exact",
                    help="with --channel awgn / rayleigh: exact or max-log bit LLRs")
    ap.add_argument("--snr-axis", choices=("reference", "esn0", "ebn0"), default=None,
                    help="what the SNR values are: the reference channel has only 'reference'; a channel model "
                         "takes esn0 or ebn0 (default ebn0, with the code's rate and the bits per symbol)")
    ap.add_argument("--puncture", default=None, metavar="COLS",
                    help="with --channel awgn / rayleigh: columns not sent and unknown to the receiver, in the "
                         "frame's order (info 0..k-1, parity k..n-1): comma-separated a, a:b or a:b:step, half-open; "
                         "a bound is an integer or k / n with +INT / -INT, e.g. k:n:6 or n-48:n")
    ap.add_argument("--shorten", default=None, metavar="COLS",
                    help="with --channel awgn / rayleigh: information columns both ends know to be 0, not sent "
                         "(the same grammar, e.g. 0:24)")
    ap.add_argument("--interleaver", default=None, metavar="SPEC",
                    help="with --channel awgn / rayleigh: bit interleaver of the transmitted bits, fixed for the run: "
                         "none, regular, block:R, random[:seed], srandom:S[:seed] or file:PATH")
    ap.add_argument("--fading-block", default=None, metavar="L|frame",
                    help="with --channel rayleigh: symbols (BPSK: bits) that share a fade (default 1); frame: one "
                         "fade per frame")
    ap.add_argument("--harq", default=None, metavar="SPEC",
                    help="with --channel awgn / rayleigh: retransmissions with combining in the frame source: "
                         "chase:R[:E] (the same E columns R times), ir:R:E (consecutive windows of E columns of the "
                         "circular buffer) or file:PATH (a transmission's columns per line); the sweep runs once per "
                         "transmission and reports FER after each, the average transmissions and the throughput")
    ap.add_argument("--harq-json", default=None, metavar="PATH",
                    help="with --harq: write the plan, the per-point HARQ figures and the counters to PATH")
    return ap


def parse_args(argv=None):
    """Parse the command line; the physical-mode options without --mode physical,
    and combinations the decoder rejects, are argparse errors."""
    from .channel import ChannelSpec
    from .device import phys_flags, phys_quant_args, phys_rule_args
    ap = build_parser()
    a = ap.parse_args(argv)
    if a.constellation is not None:
        if a.modulation is not None:
            ap.error("--constellation replaces the modulation: it takes no --modulation")
        if a.mode != "physical" or a.channel == "reference":
            ap.error("--constellation needs --mode physical --channel awgn or rayleigh")
    a.modulation = "bpsk" if a.modulation is None else a.modulation
    if a.channel == "reference" and (a.modulation != "bpsk" or a.demap != "exact"):
        ap.error("--modulation and --demap need --channel awgn or rayleigh")
    if a.mode != "physical" and (a.cn_rule != "spa" or a.schedule != "flooding" or a.alpha is not None
                                 or a.beta is not None):
        ap.error("--cn-rule, --schedule, --alpha and --beta need --mode physical")
    if a.mode != "physical" and (a.qbits is not None or a.llr_scale is not None):
        ap.error("--qbits and --llr-scale need --mode physical")
    if a.layered_tile and (a.mode != "physical" or a.schedule != "layered"):
        ap.error("--layered-tile needs --mode physical --schedule layered")
    if a.llr_scale is not None and a.qbits is None:
        ap.error("--llr-scale needs --qbits")
    if a.quant_tile and (a.mode != "physical" or a.qbits is None):
        ap.error("--quant-tile needs --mode physical --qbits")
    if a.mode != "physical" and (a.stats_json is not None or a.max_failed != 0):
        ap.error("--stats-json and --max-failed need --mode physical")
    if a.decoder != "bitflipping" and (a.bf_weight is not None or a.bf_theta is not None):
        ap.error("--bf-weight and --bf-theta need --decoder bitflipping")
    if a.decoder == "bitflipping":
        if a.mode != "physical":
            ap.error("--decoder bitflipping needs --mode physical")
        if (a.cn_rule != "spa" or a.schedule != "flooding" or a.alpha is not None or a.beta is not None
                or a.qbits is not None or a.llr_scale is not None or a.layered_tile or a.quant_tile
                or a.normalized_llr):
            ap.error("--decoder bitflipping passes no messages: --cn-rule, --schedule, --alpha, --beta, --qbits, "
                     "--llr-scale, --layered-tile, --quant-tile and --normalized-llr do not apply to it")
    a.bf_weight = 0.0 if a.bf_weight is None else a.bf_weight
    a.bf_theta = 0.0 if a.bf_theta is None else a.bf_theta
    if a.max_failed != 0 and a.stats_json is None:
        ap.error("--max-failed needs --stats-json")
    if a.max_failed < 0:
        ap.error("--max-failed must be >= 0")
    if (a.puncture is not None or a.shorten is not None) and (a.mode != "physical" or a.channel == "reference"):
        ap.error("--puncture and --shorten need --mode physical --channel awgn or rayleigh")
    if a.interleaver is not None and (a.mode != "physical" or a.channel == "reference"):
        ap.error("--interleaver needs --mode physical --channel awgn or rayleigh")
    if a.fading_block is not None and (a.mode != "physical" or a.channel != "rayleigh"):
        ap.error("--fading-block needs --mode physical --channel rayleigh")
    if a.fading_block is not None and a.fading_block.strip().lower() != "frame":
        try:
            a.fading_block = int(a.fading_block)
        except ValueError:
            ap.error(f"--fading-block takes an integer >= 1 or 'frame', got {a.fading_block!r}")
    a.fading_block = 1 if a.fading_block is None else a.fading_block
    if a.harq_json is not None and a.harq is None:
        ap.error("--harq-json needs --harq")
    if a.harq is not None:
        if a.mode != "physical" or a.channel == "reference":
            ap.error("--harq needs --mode physical --channel awgn or rayleigh")
        if a.interleaver is not None and a.interleaver.strip().lower() != "none":
            ap.error("--harq carries its own order on the air: it takes no --interleaver")
        if a.puncture is not None:
            ap.error("--harq says what is sent: it takes no --puncture (--shorten may stay)")
        if a.normalized_llr or a.output_json or a.output_csv or a.stats_json is not None:
            ap.error("--harq writes --harq-json: --normalized-llr, --output-json, --output-csv and --stats-json do "
                     "not apply to it")
    a.llr_scale = 4.0 if a.llr_scale is None else a.llr_scale
    a.alpha = 0.75 if a.alpha is None else a.alpha
    a.beta = 0.5 if a.beta is None else a.beta
    try:
        a.channel_spec = ChannelSpec(a.channel, a.modulation, a.demap)
        a.constellation_table = None
        if a.constellation is not None:
            from .constellation import parse as parse_constellation
            a.constellation_table = check_constellation_args(parse_constellation(a.constellation), a.channel_spec,
                                                             a.mode)
        a.snr_axis = check_channel_args(a.channel_spec, a.snr_axis, a.mode)
        a.interleaver, a.fading_block = check_interleave_args(a.interleaver, a.fading_block, a.channel_spec, a.mode)
        check_ira_mode(a.matrix, a.mode)
        if a.harq is not None:
            check_harq_args(a.harq, a.channel_spec, a.mode)
        check_decoder_args(a.decoder, a.bf_weight, a.bf_theta, a.mode)
        phys_flags(tile=a.layered_tile, schedule=a.schedule)
        phys_rule_args(a.cn_rule, a.schedule, a.alpha, a.beta)
        if a.qbits is not None:
            phys_quant_args(a.cn_rule, a.alpha, a.beta, a.qbits, a.llr_scale)
    except ValueError as e:
        ap.error(str(e))
    return a


def code_shape(matrix):
    """(n, k) of what --matrix names, without a device."""
    if isinstance(matrix, str) and matrix in IRA_CODES:
        from . import ira
        m, n = getattr(ira, IRA_CODES[matrix])().shape
        return n, n - m
    from .code import EncoderDecoderData, load_committed_code
    edd = EncoderDecoderData(matrix) if os.path.exists(matrix) else load_committed_code(matrix)
    return edd._n, edd._k


def cli_rate_match(a, shape=None):
    """The RateMatch of --puncture / --shorten (None without either), validated
    against the code and the modulation; ValueError otherwise.  shape: the
    code's (n, k) where the caller has it."""
    from .ratematch import RateMatch, parse_columns
    if a.puncture is None and a.shorten is None:
        return None
    n, k = shape or code_shape(a.matrix)
    rm = RateMatch(parse_columns(a.puncture, n, k) if a.puncture is not None else (),
                   parse_columns(a.shorten, n, k) if a.shorten is not None else ())
    from .constellation import effective_bps
    return rm.validate(n, k, effective_bps(a.channel_spec, a.constellation_table))


def rate_match_header(rm_info, n, k):
    """The command line's header line of a rate-matched sweep."""
    return (f"rate matching  E {rm_info['transmitted']} of n {n}  punctured {len(rm_info['punctured'])}  "
            f"shortened {len(rm_info['shortened'])}  info bits {rm_info['info_bits']} of k {k}  "
            f"effective rate {rm_info['rate']:.6f}")


def modulation_header(channel, constellation):
    """The header line's modulation field: the table's name while one is set."""
    return f"modulation {channel.modulation}" if constellation is None else f"constellation {constellation.name}"


def constellation_header(constellation):
    """The command line's header line of a sweep under a constellation table."""
    return (f"constellation {constellation.name}  bps {constellation.bps}  {len(constellation.points)} points, "
            "demapped over all of them")


def main_harq(a, snrs, rate_match, rank, world, local, allreduce, comm):
    """main() under --harq: simulate_harq and its own report."""
    from .constellation import effective_bps
    from .harq import resolve as resolve_harq
    try:  # resolved here, without a device, so that a bad plan ends before any device call
        n, k = code_shape(a.matrix)
        shortened = rate_match.shortened if rate_match is not None else ()
        plan = resolve_harq(a.harq, n, shortened).validate(
            n, shortened, effective_bps(a.channel_spec, a.constellation_table))
    except (ValueError, OSError) as e:
        raise SystemExit(f"--harq: {e}")
    res = simulate_harq(a.matrix, snrs, a.blocks, a.iterations, plan, seed=a.seed, device=local, rank=rank,
                        world=world, allreduce=allreduce, mode=a.mode, cn_rule=a.cn_rule, schedule=a.schedule,
                        alpha=a.alpha, beta=a.beta, qbits=a.qbits, llr_scale=a.llr_scale, layered_tile=a.layered_tile,
                        quant_tile=a.quant_tile, channel=a.channel_spec, snr_axis=a.snr_axis, rate_match=rate_match,
                        decoder=a.decoder, bf_weight=a.bf_weight, bf_theta=a.bf_theta, fading_block=a.fading_block,
                        constellation=a.constellation_table)
    if rank == 0:
        print(f"channel {a.channel_spec.model}  {modulation_header(a.channel_spec, a.constellation_table)}  "
              f"demap {a.channel_spec.demap}  "
              f"SNR axis {a.snr_axis}  sigma " + " ".join(f"{x:.6f}" for x in res["sigma"]))
        if a.constellation_table is not None:
            print(constellation_header(a.constellation_table))
        print(harq_header(res["plan"]))
        for pt in res["points"]:
            print(f"SNR {pt['snr_db']:.2f} dB  FER after r " + " ".join(f"{x:.6f}" for x in pt["fer_after"])
                  + f"  avg tx {pt['avg_tx']:.4f}  throughput {pt['throughput']:.4f} bit/symbol")
        if a.harq_json:
            harq_to_json(a.harq_json, a.seed, res)
    if comm is not None:
        comm.close()


def main(argv=None):
    a = parse_args(argv)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    allreduce = comm = None
    if world > 1:
        from .comm import Comm
        comm = Comm.from_env(local)
        allreduce = comm.allreduce
    snrs = snr_grid(a.initial_snr, a.end_snr, a.step_snr)
    if world > 1 and a.max_failed > 0:
        raise SystemExit("--max-failed needs a single process: failed-frame lists are not gathered across ranks")
    try:
        rate_match = cli_rate_match(a)  # the code's n and k without a device
    except ValueError as e:
        raise SystemExit(f"--puncture / --shorten: {e}")
    if a.harq is not None:
        return main_harq(a, snrs, rate_match, rank, world, local, allreduce, comm)
    interleaver = a.interleaver
    if interleaver is not None:
        try:  # resolved here, without a device, so that the header and the JSON name what ran
            n, k = code_shape(a.matrix)
            interleaver = resolve_interleaver(
                interleaver, rate_match_shape(rate_match, a.channel_spec, n, k, a.constellation_table)[0])
        except (ValueError, OSError) as e:
            raise SystemExit(f"--interleaver: {e}")
    out = simulate(a.matrix, snrs, a.blocks, a.iterations, seed=a.seed, nllr=a.normalized_llr,
                   device=local, rank=rank, world=world, allreduce=allreduce, mode=a.mode, cn_rule=a.cn_rule,
                   schedule=a.schedule, alpha=a.alpha, beta=a.beta, qbits=a.qbits, llr_scale=a.llr_scale,
                   layered_tile=a.layered_tile, quant_tile=a.quant_tile, stats=a.stats_json is not None,
                   max_failed=a.max_failed, channel=a.channel_spec, snr_axis=a.snr_axis, rate_match=rate_match,
                   decoder=a.decoder, bf_weight=a.bf_weight, bf_theta=a.bf_theta, interleaver=interleaver,
                   fading_block=a.fading_block, constellation=a.constellation_table)
    res = out[0]
    info = channel_info(a.channel_spec, a.snr_axis, snrs, res.config.rate, rate_match, res.config.n, res.config.k,
                        interleaver, a.fading_block, a.constellation_table)
    if rank == 0 and a.stats_json is not None:
        stats_to_json(a.stats_json, a.seed, out[2], channel=info)
    if rank == 0:
        print(f"channel {info['model']}  {modulation_header(a.channel_spec, a.constellation_table)}  "
              f"demap {info['demap']}  "
              f"SNR axis {info['snr_axis']}  sigma " + " ".join(f"{x:.6f}" for x in info["sigma"]))
        if a.constellation_table is not None:
            print(constellation_header(a.constellation_table))
        if "rate_match" in info:
            print(rate_match_header(info["rate_match"], res.config.n, res.config.k))
        if "interleaver" in info or "fading_block" in info:
            print(interleave_header(info))
        for sp in res.snr_points:
            print(f"SNR {sp.snr_db:.2f} dB  FER {sp.fer:.6f}  BER {sp.ber:.6e}  "
                  f"ok {sp.successful_blocks}/{sp.total_blocks}  avg conv {sp.avg_convergence_iterations:.3f}")
        if a.output_json:
            res.to_json(a.output_json)
        if a.output_csv:
            res.to_csv(a.output_csv)
    if comm is not None:
        comm.close()


if __name__ == "__main__":
    main()
