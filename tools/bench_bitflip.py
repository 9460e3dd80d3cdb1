#!/usr/bin/env python3
"""Physical mode's bit-flipping decoders next to normalized min-sum on one GPU.

wimax_2304_0.5 (or --code), the project's on-device frame source on the
reference channel at --snrs (default 0.5 and 1.0 dB), a step of --frames
frames at --iters max iterations per row, one warm-up and --steps timed steps,
all rows of a point on the same frames:
  normalized min-sum, flooding   the yardstick: its kernel is untouched by this work
  bit flipping (0, 0)            bitflip_sliced_kernel, 64 frames per workgroup
  bit flipping (0, 0) generic    bitflip_kernel, one frame per workgroup
  bit flipping (--weight, 0)     bitflip_kernel with the channel term
Every timed step runs under ldpc_profile_enable.  Prints ONE JSON line: per
SNR and row the kernel name, codewords/s (wall clock of the timed steps), FER,
average iterations, the decode kernel's nanoseconds per frame-iteration
(LDPC_K_PHYS event time / counter slot 6) and the frame source's milliseconds
per step (LDPC_K_GEN event time / steps).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))

SEED = 20260213


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--code", default="wimax_2304_0.5")
    ap.add_argument("--snrs", type=float, nargs="+", default=[0.5, 1.0])
    ap.add_argument("--frames", type=int, default=65536, help="frames per step")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row (after one warm-up)")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--weight", type=float, default=0.5, help="weight of the gradient-descent row")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)

    import numpy as np

    import ldpc_amd
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Decoder, Graph, bitflip_kernel_name, phys_kernel_name

    edd = ldpc_amd.load_committed_code(a.code)
    g = Graph(edd._h_std, device=a.device)
    pg = Graph(edd.physical_matrix(), device=a.device)
    dec = Decoder(g, a.frames)  # frame source = H_std; the fp64 message arrays are never allocated
    B = a.frames
    rows_of = [
        ("nms flooding", phys_kernel_name(pg, cn="nms"),
         lambda sig, f0: dec.phys_mc_run(pg, SEED, [sig], B, f0, a.iters, cn="nms", alpha=a.alpha)),
        ("bitflip (0,0) sliced", bitflip_kernel_name(pg),
         lambda sig, f0: dec.bitflip_mc_run(pg, SEED, [sig], B, f0, a.iters)),
        ("bitflip (0,0) generic", bitflip_kernel_name(pg, generic=True),
         lambda sig, f0: dec.bitflip_mc_run(pg, SEED, [sig], B, f0, a.iters, generic=True)),
        (f"bitflip ({a.weight:g},0)", bitflip_kernel_name(pg, a.weight),
         lambda sig, f0: dec.bitflip_mc_run(pg, SEED, [sig], B, f0, a.iters, weight=a.weight)),
    ]
    points = []
    for snr in a.snrs:
        sig = mc.sigma_for_snr(snr)
        rows = []
        for label, kernel, run in rows_of:
            run(sig, 0)  # warm-up
            dec.profile_read()
            dec.profile(True)
            tot = np.zeros(7, np.int64)
            t0 = time.perf_counter()
            for s in range(a.steps):
                tot += run(sig, (s + 1) * B)[0]
            dt = time.perf_counter() - t0
            dec.profile(False)
            prof = dec.profile_read()
            pms, launches = prof["phys"]
            frames = int(tot[0])
            rows.append({
                "row": label, "kernel": kernel, "cw_per_s": frames / dt, "fer": int(tot[1]) / frames,
                "avg_iters": int(tot[6]) / frames, "kernel_ms": pms, "launches": int(launches),
                "kernel_ns_per_frame_iteration": 1e6 * pms / max(int(tot[6]), 1),
                "generate_ms_per_step": prof["generate"][0] / a.steps, "step_ms": 1e3 * dt / a.steps})
        points.append({"snr_db": snr, "rows": rows})
    dec.close()
    print(json.dumps({"tool": "bench_bitflip", "code": a.code, "frames_per_step": B, "steps": a.steps,
                      "max_iter": a.iters, "alpha": a.alpha, "weight": a.weight, "points": points}))


if __name__ == "__main__":
    main()
