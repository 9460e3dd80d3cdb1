#!/usr/bin/env python3
"""What a HARQ plan costs the physical-mode frame source on one GPU.

wimax_2304_0.5 (65,536-frame steps, the frame source's row form) and the
DVB-S2 profile (8,192-frame steps, its tile form), normalized min-sum layered
at --iters max iterations, under AWGN/16-QAM exact and Rayleigh/16-QAM exact,
with no plan, a one-transmission plan (chase:1: every column once, the frames
of no plan through the accumulator), and ir:2:n/2 and ir:4:n/2 (every column
once and twice) in one run: the event time of the `generate` kind per step
(ldpc_profile_enable) and codewords/s by the host clock with profiling off.

sigma is that of --ebn0 at the mother code's rate k / n for every row (the
defaults lie inside the no-plan waterfall); the ir:4 rows, whose columns each
arrive twice, run 3 dB lower under AWGN and 4 to 5 dB lower under Rayleigh
fading (two independent fades per column; EBN0_IR4_OFFSET) so that they too
decode inside a waterfall.

Prints ONE JSON line.

--no-plan-only --package-dir OTHER_TREE/ldpc-simulator_amd runs the no-plan rows
alone against another build of the package (an A/B of the untouched path; the
other build needs none of the HARQ API).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEED = 20260213
CHANNELS = {"awgn-qam16-exact": ("awgn", "qam16", "exact"), "rayleigh-qam16-exact": ("rayleigh", "qam16", "exact")}
EBN0 = {"wimax_2304_0.5:awgn-qam16-exact": 3.6, "wimax_2304_0.5:rayleigh-qam16-exact": 6.0,
        "dvbs2_profile_64800_0.5:awgn-qam16-exact": 4.1, "dvbs2_profile_64800_0.5:rayleigh-qam16-exact": 8.08}
CODES = {"wimax_2304_0.5": 65536, "dvbs2_profile_64800_0.5": 8192}
EBN0_IR4_OFFSET = {"wimax_2304_0.5:awgn-qam16-exact": -3.0, "wimax_2304_0.5:rayleigh-qam16-exact": -4.0,
                   "dvbs2_profile_64800_0.5:awgn-qam16-exact": -3.0, "dvbs2_profile_64800_0.5:rayleigh-qam16-exact": -5.0}
# (name, transmissions, positions each as a fraction of n)
PLANS = (("none", 0, 0.0), ("chase:1", 1, 1.0), ("ir:2:n/2", 2, 0.5), ("ir:4:n/2", 4, 0.5))


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


def bench(a, ebn0_of):
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
            run(sigma)  # warm-up (and, under a plan, the accumulator's allocation)
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
            for plan_name, R, frac in (PLANS[:1] if a.no_plan_only else PLANS):
                info = None
                if R:
                    from ldpc_amd.harq import HarqPlan
                    plan = HarqPlan.circular(n, R, int(n * frac), int(n * frac) if R > 1 else 0)
                    dec.set_harq(plan)
                    info = plan.info()
                ebn0 = ebn0_of[f"{code}:{name}"] + (EBN0_IR4_OFFSET[f"{code}:{name}"] if R == 4 else 0.0)
                sigma = sigma_for_ebn0(ebn0, k / n, cs.bps)
                row = {"channel": name, "plan": plan_name, "harq": info, "ebn0_db": ebn0, "sigma": sigma}
                row.update(measure(sigma))
                rows.append(row)
                if R:
                    dec.set_harq(None)
            for r in rows:
                if r["channel"] == name:
                    r["generate_vs_none"] = r["generate_ms_median"] / next(
                        q for q in rows if q["channel"] == name and q["harq"] is None)["generate_ms_median"]
        dec.set_channel(None)
        dec.close()
        codes.append({"code": code, "n": n, "k": k, "frames_per_step": B, "rows": rows})
    return codes


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--codes", nargs="+", default=list(CODES), choices=list(CODES))
    ap.add_argument("--channels", nargs="+", default=list(CHANNELS), choices=list(CHANNELS))
    ap.add_argument("--frames", type=int, default=None, help="frames per step (default: 65536 / 8192 by code)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row and kind of timing, after one warm-up")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--ebn0", nargs="*", default=[], metavar="CODE:CHANNEL=DB", help="the no-plan rows' Eb/N0")
    ap.add_argument("--no-plan-only", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--package-dir", default=os.path.join(ROOT, "ldpc-simulator_amd"),
                    help="directory holding the ldpc_amd package to measure")
    a = ap.parse_args(argv)
    sys.path.insert(0, a.package_dir)
    ebn0_of = dict(EBN0)
    for item in a.ebn0:
        key, _, val = item.partition("=")
        ebn0_of[key] = float(val)
    out = {"tool": "bench_phys_harq", "package_dir": os.path.relpath(a.package_dir, ROOT), "max_iter": a.iters,
           "alpha": a.alpha, "steps": a.steps, "rule": "nms-layered", "codes": bench(a, ebn0_of)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
