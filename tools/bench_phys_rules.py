#!/usr/bin/env python3
"""Physical mode's check rules and schedules side by side on one GPU.

wimax_2304_0.5 (or --code), the project's on-device frame source, the two SNR
points bench.py uses for physical mode (-2.5 dB in the waterfall, 1.0 dB), a
step of --frames frames at --iters max iterations per configuration:
sum-product flooding, normalized min-sum flooding, normalized min-sum layered,
and (--qbits, default 6; 0 skips them) the fixed-point normalized min-sum
decoder under both schedules on the same frames, in each point's "quantized"
rows.
Every timed step runs under ldpc_profile_enable.  Prints ONE JSON line: per
SNR and configuration the kernel name, codewords/s (wall clock of the timed
steps), FER, average iterations and the decode kernel's milliseconds per
frame-iteration (LDPC_K_PHYS event time / counter slot 6).

The yardstick is the sum-product flooding row of the same run on the same
GPU -- that kernel is untouched by the min-sum work; the yardstick of a
quantized row is the fp32 min-sum row of the same schedule.  LDPC_LAYERED_NT and
LDPC_LAYERED_PER_CU (read by the library per launch) override the layered
kernel's block size and workgroups per CU for A/B runs of this tool.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))

SEED = 20260213
CONFIGS = (("spa", "flooding"), ("nms", "flooding"), ("nms", "layered"))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--code", default="wimax_2304_0.5")
    ap.add_argument("--snrs", type=float, nargs="+", default=[-2.5, 1.0])
    ap.add_argument("--frames", type=int, default=65536, help="frames per step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per configuration (after one warm-up)")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mc-stats", type=int, default=None, metavar="MAX_FAILED",
                    help="collect the Monte-Carlo statistics (Decoder.mc_stats) with this many failed-frame records "
                         "per point: the cost of statistics on (default: off)")
    ap.add_argument("--configs", nargs="+", default=["-".join(c) for c in CONFIGS],
                    choices=["-".join(c) for c in CONFIGS], help="rule-schedule pairs to run")
    ap.add_argument("--qbits", type=int, default=6, help="message bits of the quantized rows (0: none)")
    ap.add_argument("--llr-scale", type=float, default=4.0, help="quantizer steps per unit of LLR")
    a = ap.parse_args(argv)

    import numpy as np

    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Decoder, Graph, phys_kernel_name

    edd = ldpc_amd.load_committed_code(a.code)
    g = Graph(edd._h_std, device=a.device)
    pg = Graph(edd.physical_matrix(), device=a.device)
    dec = Decoder(g, a.frames)  # frame source = H_std; the fp64 message arrays are never allocated
    if a.mc_stats is not None:
        dec.mc_stats(True, a.mc_stats)
    B = a.frames
    points = []
    for snr in a.snrs:
        sig = mc.sigma_for_snr(snr)
        rows, qrows = [], []
        runs = [(c.split("-"), {}) for c in a.configs]
        if a.qbits:
            runs += [(("nms", sch), dict(qbits=a.qbits, llr_scale=a.llr_scale)) for sch in ("flooding", "layered")]
        for (cn, schedule), q in runs:
            kw = dict(cn=cn, schedule=schedule, alpha=a.alpha, **q)
            dec.phys_mc_run(pg, SEED, [sig], B, 0, a.iters, **kw)  # warm-up (builds the layer table)
            dec.profile_read()
            dec.profile(True)
            tot = np.zeros(7, np.int64)
            t0 = time.perf_counter()
            for s in range(a.steps):
                tot += dec.phys_mc_run(pg, SEED, [sig], B, (s + 1) * B, a.iters, **kw)[0]
            dt = time.perf_counter() - t0
            dec.profile(False)
            pms, launches = dec.profile_read()["phys"]
            frames = int(tot[0])
            (qrows if q else rows).append({
                "cn": cn, "schedule": schedule, **q, "kernel": phys_kernel_name(pg, cn=cn, schedule=schedule, **q),
                "cw_per_s": frames / dt, "fer": int(tot[1]) / frames, "avg_iters": int(tot[6]) / frames,
                "kernel_ms": pms, "launches": int(launches),
                "kernel_ms_per_frame_iteration": pms / max(int(tot[6]), 1)})
        points.append({"snr_db": snr, "configs": rows, **({"quantized": qrows} if qrows else {})})
    dec.close()
    print(json.dumps({"tool": "bench_phys_rules", "code": a.code, "frames_per_step": B, "steps": a.steps,
                      "max_iter": a.iters, "alpha": a.alpha, "mc_stats": a.mc_stats, "points": points}))  # quantized rows: alpha_q = round(16 alpha)


if __name__ == "__main__":
    main()
