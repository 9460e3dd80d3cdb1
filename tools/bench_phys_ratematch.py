#!/usr/bin/env python3
"""What rate matching costs the physical-mode frame source on one GPU.

wimax_2304_0.5 (65,536-frame steps) and the DVB-S2 profile (8,192-frame steps),
normalized min-sum layered at --iters max iterations, under AWGN/BPSK and
AWGN/64-QAM exact, each without a pattern and with the tests' wimax_576_0.5
pattern scaled to the code: every sixth parity column punctured ("k:n:6") and
the first k/12 information bits shortened ("0:k/12"); E = 7/8 n, effective rate
11/21.  The no-pattern row runs at --ebn0 (defaults inside the waterfall: wimax
1.0 dB BPSK and 6.0 dB 64-QAM, the DVB-S2 profile 2.0 and 6.55 dB); the
pattern's row runs at the Eb/N0 (on its own effective rate) a bisection on
--calib-frames frames finds for the no-pattern row's average iteration count,
so the decoders do comparable work and the rows differ by their frame source.

Per row, after one warm-up step: --steps steps timed by the host clock with
profiling off (codewords/s: the median step), then --steps steps under
ldpc_profile_enable for the event time of the `generate` kind.  Prints ONE JSON
line.

--no-pattern-only --package-dir OTHER_TREE/ldpc-simulator_amd runs the
no-pattern rows alone against another build of the package (an A/B of the
no-pattern path; the other build needs none of the rate-matching API).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 20260213
CHANNELS = {"awgn-bpsk": ("awgn", "bpsk", "exact"), "awgn-qam64-exact": ("awgn", "qam64", "exact")}
EBN0 = {"wimax_2304_0.5:awgn-bpsk": 1.0, "wimax_2304_0.5:awgn-qam64-exact": 6.0,
        "dvbs2_profile_64800_0.5:awgn-bpsk": 2.0, "dvbs2_profile_64800_0.5:awgn-qam64-exact": 6.55}
CODES = {"wimax_2304_0.5": 65536, "dvbs2_profile_64800_0.5": 8192}


def scaled_pattern(n, k):
    """(punctured, shortened): the tests' wimax_576_0.5 pattern at this code's size."""
    return tuple(range(k, n, 6)), tuple(range(k // 12))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--channels", nargs="+", default=list(CHANNELS), choices=list(CHANNELS))
    ap.add_argument("--frames", type=int, default=None, help="frames per step (default: 65536 / 8192 by code)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row and kind of timing, after one warm-up")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--ebn0", nargs="*", default=[], metavar="CODE:CHANNEL=DB", help="the no-pattern rows' Eb/N0")
    ap.add_argument("--calib-frames", type=int, default=None, help="frames of a calibration run (default: a step / 16)")
    ap.add_argument("--no-pattern-only", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "ldpc-simulator_amd"),
                    help="directory holding the ldpc_amd package to measure")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.package_dir)
    ebn0_of = dict(EBN0)
    for item in a.ebn0:
        key, _, val = item.partition("=")
        ebn0_of[key] = float(val)

    import numpy as np

    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
    from ldpc_amd.device import Decoder, Graph

    out = {"tool": "bench_phys_ratematch", "package_dir": os.path.relpath(a.package_dir, ROOT), "max_iter": a.iters,
           "alpha": a.alpha, "steps": a.steps, "rule": "nms-layered", "codes": []}
    for code in a.codes:
        B = a.frames or CODES[code]
        if code in mc.IRA_CODES:
            from ldpc_amd import ira
            H = getattr(ira, mc.IRA_CODES[code])()
            g = pg = Graph(H, device=a.device)
            n, k = H.shape[1], H.shape[1] - H.shape[0]
        else:
            edd = ldpc_amd.load_committed_code(code)
            g, pg = Graph(edd._h_std, device=a.device), Graph(edd.physical_matrix(), device=a.device)
            n, k = edd._n, edd._k
        dec = Decoder(g, B)
        calib = a.calib_frames or max(256, B // 16)
        base = [0]

        def run(sigma, frames):
            base[0] += frames  # fresh frames every step
            return dec.phys_mc_run(pg, SEED, [sigma], frames, base[0], a.iters, cn="nms", schedule="layered",
                                   alpha=a.alpha)[0]

        def measure(sigma):
            run(sigma, B)  # warm-up
            tot, wall = np.zeros(7, np.int64), []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                tot += run(sigma, B)  # returns after the counters are copied back: the device is idle
                wall.append(time.perf_counter() - t0)
            dec.profile_read()
            dec.profile(True)
            gen, prof_wall = [], []
            for _ in range(a.steps):
                t0 = time.perf_counter()
                run(sigma, B)
                prof_wall.append(time.perf_counter() - t0)
                gen.append(dec.profile_read()["generate"][0])
            dec.profile(False)
            frames = int(tot[0])
            return {"cw_per_s": B / statistics.median(wall), "step_ms": [1e3 * w for w in wall],
                    "fer": int(tot[1]) / frames, "avg_iters": int(tot[6]) / frames,
                    "generate_ms": gen, "generate_ms_median": statistics.median(gen),
                    "generate_share_of_profiled_step": statistics.median(gen) / (1e3 * statistics.median(prof_wall))}

        rows = []
        for name in a.channels:
            cs = ChannelSpec(*CHANNELS[name])
            dec.set_channel(cs)
            ebn0 = ebn0_of[f"{code}:{name}"]
            sigma = sigma_for_ebn0(ebn0, k / n, cs.bps)
            row = {"channel": name, "pattern": None, "transmitted": n, "info_bits": k, "rate": k / n,
                   "ebn0_db": ebn0, "sigma": sigma}
            row.update(measure(sigma))
            rows.append(row)
            if a.no_pattern_only:
                continue
            from ldpc_amd.ratematch import RateMatch
            rm = RateMatch(*scaled_pattern(n, k)).validate(n, k, cs.bps)
            rate = rm.effective_rate(n, k)
            dec.set_rate_match(rm)
            lo, hi = -2.0, 30.0  # average iterations fall as Eb/N0 rises
            for _ in range(12):
                ebn0 = 0.5 * (lo + hi)
                it = int(run(sigma_for_ebn0(ebn0, rate, cs.bps), calib)[6]) / calib
                lo, hi = (ebn0, hi) if it > row["avg_iters"] else (lo, ebn0)
            ebn0 = round(0.5 * (lo + hi), 2)
            sigma = sigma_for_ebn0(ebn0, rate, cs.bps)
            prow = {"channel": name, "pattern": {"punctured": "k:n:6", "shortened": "0:k/12",
                                                 "n_punct": len(rm.punctured), "n_short": len(rm.shortened)},
                    "transmitted": rm.n_transmitted(n), "info_bits": rm.info_bits(k), "rate": rate, "ebn0_db": ebn0,
                    "ebn0_db_from": f"bisection on {calib} frames", "sigma": sigma}
            prow.update(measure(sigma))
            rows.append(prow)
            dec.set_rate_match(None)
        dec.set_channel(None)
        dec.close()
        out["codes"].append({"code": code, "n": n, "k": k, "frames_per_step": B, "rows": rows})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
