#!/usr/bin/env python3
"""What the physical-mode channel models cost on one GPU.

wimax_2304_0.5 (65,536-frame steps) and the DVB-S2 profile (8,192-frame steps),
normalized min-sum layered at --iters max iterations, under five channels:
the reference channel, AWGN/BPSK, AWGN/64-QAM exact, AWGN/64-QAM max-log and
Rayleigh/16-QAM exact.  The reference row runs at --ref-snr on its own axis
(-2.5 dB, the waterfall point bench.py times); every other row runs at the
Eb/N0 a bisection on --calib-frames frames finds for the reference row's
average iteration count (--ebn0 CODE:CHANNEL=dB ... skips the search for a
row), so that the decoders do comparable work and the rows differ by their
frame source.  The Eb/N0 values are part of the output.

Per row, after one warm-up step: --steps steps timed by the host clock with
profiling off (codewords/s: the median step), then --steps steps under
ldpc_profile_enable for the event time of the `generate` kind and its share
of the profiled step.  Prints ONE JSON line.

--channels reference --package-dir OTHER_TREE/ldpc-simulator_amd runs the
reference row alone against another build of the package (an A/B of the
untouched reference kernels; the other build needs none of the channel API).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 20260213
CHANNELS = {  # name -> (model, modulation, demap), None = the reference channel
    "reference": None,
    "awgn-bpsk": ("awgn", "bpsk", "exact"),
    "awgn-qam64-exact": ("awgn", "qam64", "exact"),
    "awgn-qam64-maxlog": ("awgn", "qam64", "maxlog"),
    "rayleigh-qam16-exact": ("rayleigh", "qam16", "exact"),
}
CODES = {"wimax_2304_0.5": 65536, "dvbs2_profile_64800_0.5": 8192}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--channels", nargs="+", default=list(CHANNELS), choices=list(CHANNELS))
    ap.add_argument("--frames", type=int, default=None, help="frames per step (default: 65536 / 8192 by code)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row and kind of timing, after one warm-up")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--ref-snr", type=float, default=-2.5, help="the reference row's point on the reference axis (dB)")
    ap.add_argument("--calib-frames", type=int, default=None, help="frames of a calibration run (default: a step / 16)")
    ap.add_argument("--ebn0", nargs="*", default=[], metavar="CODE:CHANNEL=DB", help="fix a row's Eb/N0 instead")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "ldpc-simulator_amd"),
                    help="directory holding the ldpc_amd package to measure")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.package_dir)
    fixed = {}
    for item in a.ebn0:
        key, _, val = item.partition("=")
        fixed[key] = float(val)

    import numpy as np

    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Decoder, Graph

    out = {"tool": "bench_phys_channel", "package_dir": os.path.relpath(a.package_dir, ROOT), "max_iter": a.iters,
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
            gen, prof_wall, kinds = [], [], {}
            for _ in range(a.steps):
                t0 = time.perf_counter()
                run(sigma, B)
                prof_wall.append(time.perf_counter() - t0)
                p = dec.profile_read()
                gen.append(p["generate"][0])
                for kind, (ms, cnt) in p.items():
                    if cnt:
                        kinds[kind] = kinds.get(kind, 0.0) + ms / a.steps
            dec.profile(False)
            frames = int(tot[0])
            return {"cw_per_s": B / statistics.median(wall), "step_ms": [1e3 * w for w in wall],
                    "fer": int(tot[1]) / frames, "avg_iters": int(tot[6]) / frames,
                    "generate_ms": gen, "generate_ms_median": statistics.median(gen),
                    "generate_share_of_profiled_step": statistics.median(gen) / (1e3 * statistics.median(prof_wall)),
                    "kind_ms_per_step": kinds}

        rows, target = [], None
        for name in a.channels:
            spec = CHANNELS[name]
            if spec is None:
                dec_sigma = mc.sigma_for_snr(a.ref_snr)
                row = {"channel": name, "snr_axis": "reference", "snr_db": a.ref_snr, "sigma": dec_sigma}
            else:
                from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
                cs = ChannelSpec(*spec)
                dec.set_channel(cs)
                key = f"{code}:{name}"
                if key in fixed:
                    ebn0, how = fixed[key], "given"
                else:
                    if target is None:
                        raise SystemExit("the Eb/N0 search needs the reference row first (or --ebn0 for every row)")
                    lo, hi = -2.0, 30.0  # average iterations fall as Eb/N0 rises
                    for _ in range(12):
                        ebn0 = 0.5 * (lo + hi)
                        it = int(run(sigma_for_ebn0(ebn0, k / n, cs.bps), calib)[6]) / calib
                        lo, hi = (ebn0, hi) if it > target else (lo, ebn0)
                    ebn0, how = round(0.5 * (lo + hi), 2), f"bisection on {calib} frames"
                dec_sigma = sigma_for_ebn0(ebn0, k / n, cs.bps)
                row = {"channel": name, "snr_axis": "ebn0", "snr_db": ebn0, "snr_db_from": how, "sigma": dec_sigma}
            row.update(measure(dec_sigma))
            if spec is None:
                target = row["avg_iters"]
            else:
                dec.set_channel(None)
            rows.append(row)
        dec.close()
        out["codes"].append({"code": code, "n": n, "k": k, "frames_per_step": B, "rows": rows})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
