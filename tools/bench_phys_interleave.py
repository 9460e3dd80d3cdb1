#!/usr/bin/env python3
"""What a bit interleaver costs the physical-mode frame source on one GPU, and
what it buys under block fading.

(a) --part gen: wimax_2304_0.5 (65,536-frame steps, the frame source's row
form) and the DVB-S2 profile (8,192-frame steps, its tile form), normalized
min-sum layered at --iters max iterations, under AWGN/16-QAM and AWGN/64-QAM
exact at --ebn0 (defaults inside the waterfall), with the interleaver none /
regular / random:7 in one run: the event time of the `generate` kind per step
(ldpc_profile_enable) and codewords/s by the host clock with profiling off.
The interleaved rows differ from the no-interleaver row of the same run by the
gathers of the codeword bits and the scattered stores of the LLRs (and, on this
memoryless channel, by nothing the decoder can see beyond which columns share a
symbol).

(b) --part fer: FER against Eb/N0 on wimax_2304_0.5, normalized min-sum
layered, Rayleigh/16-QAM exact, coherence length 1 / 24 / frame, each without
an interleaver and with the regular one (--fer-interleavers adds others);
--fer-frames frames per point.

Prints ONE JSON line.

--no-option-only --package-dir OTHER_TREE/ldpc-simulator_amd runs part (a)'s
no-interleaver rows alone against another build of the package (an A/B of the
untouched path; the other build needs none of the interleaver API).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 20260213
CHANNELS = {"awgn-qam16-exact": ("awgn", "qam16", "exact"), "awgn-qam64-exact": ("awgn", "qam64", "exact")}
EBN0 = {"wimax_2304_0.5:awgn-qam16-exact": 3.6, "wimax_2304_0.5:awgn-qam64-exact": 6.0,
        "dvbs2_profile_64800_0.5:awgn-qam16-exact": 4.1, "dvbs2_profile_64800_0.5:awgn-qam64-exact": 6.55}
CODES = {"wimax_2304_0.5": 65536, "dvbs2_profile_64800_0.5": 8192}
INTERLEAVERS = ("none", "regular", "random:7")
FER_CODE = "wimax_2304_0.5"
FER_BLOCKS = (1, 24, "frame")


def load(code, device):
    """(frame-source graph, decoding graph, n, k) of a committed or IRA code."""
    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Graph
    if code in mc.IRA_CODES:
        from ldpc_amd import ira
        H = getattr(ira, mc.IRA_CODES[code])()
        g = Graph(H, device=device)
        return g, g, H.shape[1], H.shape[1] - H.shape[0]
    edd = ldpc_amd.load_committed_code(code)
    return Graph(edd._h_std, device=device), Graph(edd.physical_matrix(), device=device), edd._n, edd._k


def part_gen(a, ebn0_of):
    import numpy as np

    from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
    from ldpc_amd.device import Decoder

    codes = []
    for code in a.codes:
        B = a.frames or CODES[code]
        g, pg, n, k = load(code, a.device)
        dec = Decoder(g, B)
        base = [0]

        def run(sigma):
            base[0] += B  # fresh frames every step
            return dec.phys_mc_run(pg, SEED, [sigma], B, base[0], a.iters, cn="nms", schedule="layered",
                                   alpha=a.alpha)[0]

        def measure(sigma):
            run(sigma)  # warm-up
            tot, wall = np.zeros(7, np.int64), []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                tot += run(sigma)  # returns after the counters are copied back: the device is idle
                wall.append(time.perf_counter() - t0)
            dec.profile_read()
            dec.profile(True)
            gen = []
            for _ in range(a.steps):
                run(sigma)
                gen.append(dec.profile_read()["generate"][0])
            dec.profile(False)
            frames = int(tot[0])
            return {"cw_per_s": B / statistics.median(wall), "step_ms": [1e3 * w for w in wall],
                    "fer": int(tot[1]) / frames, "avg_iters": int(tot[6]) / frames,
                    "generate_ms": gen, "generate_ms_median": statistics.median(gen)}

        rows = []
        for name in a.channels:
            cs = ChannelSpec(*CHANNELS[name])
            dec.set_channel(cs)
            ebn0 = ebn0_of[f"{code}:{name}"]
            sigma = sigma_for_ebn0(ebn0, k / n, cs.bps)
            for spec in (("none",) if a.no_option_only else INTERLEAVERS):
                info = None
                if spec != "none":
                    from ldpc_amd import interleave
                    ilv = interleave.parse(spec, n)
                    dec.set_interleaver(ilv)
                    info = ilv.info()
                row = {"channel": name, "interleaver": info, "ebn0_db": ebn0, "sigma": sigma}
                row.update(measure(sigma))
                rows.append(row)
                if spec != "none":
                    dec.set_interleaver(None)
            for r in rows:
                if r["channel"] == name:
                    r["generate_vs_none"] = r["generate_ms_median"] / next(
                        q for q in rows if q["channel"] == name and q["interleaver"] is None)["generate_ms_median"]
        dec.set_channel(None)
        dec.close()
        codes.append({"code": code, "n": n, "k": k, "frames_per_step": B, "rows": rows})
    return codes


def part_fer(a):
    from ldpc_amd import interleave
    from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
    from ldpc_amd.device import Decoder

    g, pg, n, k = load(FER_CODE, a.device)
    cs = ChannelSpec("rayleigh", "qam16", "exact")
    ebn0 = [a.fer_ebn0[0] + i * a.fer_ebn0[2] for i in range(int(round((a.fer_ebn0[1] - a.fer_ebn0[0]) / a.fer_ebn0[2])) + 1)]
    sigmas = [sigma_for_ebn0(e, k / n, cs.bps) for e in ebn0]
    dec = Decoder(g, min(a.fer_frames, 65536))
    dec.set_channel(cs)
    curves = []
    for block in FER_BLOCKS:
        dec.set_fading_block(2 ** 31 - 1 if block == "frame" else block)
        for spec in a.fer_interleavers:
            ilv = interleave.parse(spec, n)
            dec.set_interleaver(ilv)
            ctr = dec.phys_mc_run(pg, SEED, sigmas, a.fer_frames, 0, a.iters, cn="nms", schedule="layered", alpha=a.alpha)
            curves.append({"fading_block": block, "interleaver": None if ilv is None else ilv.info(),
                           "frames": [int(c[0]) for c in ctr], "failed": [int(c[1]) for c in ctr],
                           "fer": [int(c[1]) / int(c[0]) for c in ctr],
                           "avg_iters": [int(c[6]) / int(c[0]) for c in ctr]})
    dec.set_interleaver(None)
    dec.set_fading_block(1)
    dec.set_channel(None)
    dec.close()
    return {"code": FER_CODE, "n": n, "k": k, "channel": "rayleigh-qam16-exact", "symbols_per_frame": n // cs.bps,
            "ebn0_db": ebn0, "curves": curves}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--part", choices=("gen", "fer", "both"), default="both")
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--channels", nargs="+", default=list(CHANNELS), choices=list(CHANNELS))
    ap.add_argument("--frames", type=int, default=None, help="frames per step (default: 65536 / 8192 by code)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row and kind of timing, after one warm-up")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--ebn0", nargs="*", default=[], metavar="CODE:CHANNEL=DB", help="part (a)'s Eb/N0")
    ap.add_argument("--fer-ebn0", nargs=3, type=float, default=[6.0, 20.0, 2.0], metavar=("FIRST", "LAST", "STEP"))
    ap.add_argument("--fer-interleavers", nargs="+", default=["none", "regular"], metavar="SPEC",
                    help="part (b): the interleavers of the curves (ldpc_amd.interleave.parse)")
    ap.add_argument("--fer-frames", type=int, default=16384, help="part (b): frames per Eb/N0 point")
    ap.add_argument("--no-option-only", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "ldpc-simulator_amd"),
                    help="directory holding the ldpc_amd package to measure")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.package_dir)
    ebn0_of = dict(EBN0)
    for item in a.ebn0:
        key, _, val = item.partition("=")
        ebn0_of[key] = float(val)
    out = {"tool": "bench_phys_interleave", "package_dir": os.path.relpath(a.package_dir, ROOT), "max_iter": a.iters,
           "alpha": a.alpha, "steps": a.steps, "rule": "nms-layered"}
    if a.part in ("gen", "both") or a.no_option_only:
        out["codes"] = part_gen(a, ebn0_of)
    if a.part in ("fer", "both") and not a.no_option_only:
        out["fer"] = part_fer(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
