#!/usr/bin/env python3
"""What a constellation table costs the physical-mode frame source on one GPU.

wimax_2304_0.5 (fp32 rows, 65,536-frame steps) and the DVB-S2 profile (fp32
tiles, 8,192-frame steps), normalized min-sum layered at --iters max
iterations, AWGN, exact and max-log, under five symbol kinds:
  qam16        the built-in 16-QAM (per-axis kernels)
  qam16-table  the same 16-QAM written out as a table: the same frames, so the
               difference is the price of generality
  8psk, 16apsk the built-in tables
  rand32       a seeded random 32-point table (bps = 5); where n is no
               multiple of 5 the last n % 5 parity columns are punctured
               (wimax_2304_0.5: 4 columns, E = 2300, through the pattern path)
The qam16 row runs at --ebn0 (dB); every other row runs at the Eb/N0 a
bisection on --calib-frames frames finds for that row's average iteration
count (--fix CODE:ROW=dB skips the search for a row), so that the decoders do
comparable work and the rows differ by their frame source.  The max-log rows
reuse the exact rows' Eb/N0.

Per row, after one warm-up step: --steps steps timed by the host clock with
profiling off (codewords/s: the median step), then --steps steps under
ldpc_profile_enable for the event time of the `generate` kind and its share
of the profiled step.  Prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 20260213
ROWS = ("qam16", "qam16-table", "8psk", "16apsk", "rand32")
CODES = {"wimax_2304_0.5": 65536, "dvbs2_profile_64800_0.5": 8192}


def tables():
    """name -> Constellation (None: the built-in modulation)."""
    import numpy as np

    from ldpc_amd.constellation import Constellation
    d = 1.0 / 10.0 ** 0.5
    axis = {(0, 0): -3 * d, (0, 1): -d, (1, 1): d, (1, 0): 3 * d}  # the channel models' Gray axis
    qam = [complex(axis[(a >> 3) & 1, (a >> 2) & 1], axis[(a >> 1) & 1, a & 1]) for a in range(16)]
    rng = np.random.default_rng(32)
    rand = list(rng.normal(size=32) + 1j * rng.normal(size=32))
    return {"qam16": None, "qam16-table": Constellation.from_points(qam, name="qam16-table", normalize=False),
            "8psk": Constellation.psk8(), "16apsk": Constellation.apsk16(),
            "rand32": Constellation.from_points(rand, name="rand32")}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    ap.add_argument("--demaps", nargs="+", default=["exact", "maxlog"], choices=["exact", "maxlog"])
    ap.add_argument("--frames", type=int, default=None, help="frames per step (default: 65536 / 8192 by code)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row and kind of timing, after one warm-up")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--ebn0", type=float, default=5.0, help="the qam16 row's Eb/N0 (dB)")
    ap.add_argument("--calib-frames", type=int, default=None, help="frames of a calibration run (default: a step / 16)")
    ap.add_argument("--fix", nargs="*", default=[], metavar="CODE:ROW=DB", help="fix a row's Eb/N0 instead")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))
    fixed = {}
    for item in a.fix:
        key, _, val = item.partition("=")
        fixed[key] = float(val)

    import numpy as np

    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.channel import ChannelSpec, sigma_for_ebn0
    from ldpc_amd.device import Decoder, Graph
    from ldpc_amd.ratematch import RateMatch

    tabs = tables()
    out = {"tool": "bench_phys_constellation", "max_iter": a.iters, "alpha": a.alpha, "steps": a.steps,
           "rule": "nms-layered", "model": "awgn", "codes": []}
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

        rows, target, ebn0_of = [], None, {}
        for demap in a.demaps:
            for name in a.rows:
                tab = tabs[name]
                bps = 4 if tab is None else tab.bps
                dec.set_channel(ChannelSpec("awgn", "qam16" if tab is None else "bpsk", demap))
                dec.set_constellation(tab)
                cut = n % bps  # columns no whole symbol is left for
                dec.set_rate_match(RateMatch(tuple(range(n - cut, n)), ()) if cut else None)
                rate = k / (n - cut)
                key = f"{code}:{name}"
                if name == "qam16":
                    ebn0, how = a.ebn0, "given"
                elif key in fixed:
                    ebn0, how = fixed[key], "given"
                elif name in ebn0_of:
                    ebn0, how = ebn0_of[name], "the exact row's"
                else:
                    if target is None:
                        raise SystemExit("the Eb/N0 search needs the qam16 row first (or --fix for every row)")
                    lo, hi = -2.0, 30.0  # average iterations fall as Eb/N0 rises
                    for _ in range(12):
                        ebn0 = 0.5 * (lo + hi)
                        it = int(run(sigma_for_ebn0(ebn0, rate, bps, table=True), calib)[6]) / calib
                        lo, hi = (ebn0, hi) if it > target else (lo, ebn0)
                    ebn0, how = round(0.5 * (lo + hi), 2), f"bisection on {calib} frames"
                ebn0_of.setdefault(name, ebn0)
                sigma = sigma_for_ebn0(ebn0, rate, bps, table=True)
                row = {"row": name, "demap": demap, "bps": bps, "snr_axis": "ebn0", "snr_db": ebn0, "snr_db_from": how,
                       "sigma": sigma, "punctured": cut}
                row.update(measure(sigma))
                if name == "qam16" and target is None:
                    target = row["avg_iters"]
                rows.append(row)
        dec.set_rate_match(None)
        dec.set_constellation(None)
        dec.set_channel(None)
        dec.close()
        out["codes"].append({"code": code, "n": n, "k": k, "frames_per_step": B, "rows": rows})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
