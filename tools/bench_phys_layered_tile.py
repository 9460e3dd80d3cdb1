#!/usr/bin/env python3
"""The layered min-sum schedule on the HBM tile kernels, measured on one GPU.

Two comparisons, each on the project's on-device frames, one warm-up and
--steps timed steps per row under ldpc_profile_enable:

  dvbs2  the DVB-S2-profile code (n = 64800, ldpc_amd/ira.py; the graph is its
         own frame source), --dvbs2-frames frames per step (bench.py's config 5
         uses 8192), normalized min-sum: flooding on the HBM tile kernels
         (phys_cn_tile_kernel / phys_vn_tile_kernel -- the yardstick, untouched
         by the layered work) against layered (phys_layer_tile_kernel, chosen
         automatically: a frame's state does not fit LDS), same frames.
  wimax  wimax_2304_0.5, --wimax-frames frames per step, normalized min-sum
         layered: the LDS kernel (phys_layered_kernel, the default) against
         the tile kernels forced with LDPC_F_LAYERED_TILE.  Report only.

Per SNR and row: kernel name, codewords/s (wall clock of the timed steps), FER,
average iterations and the decode kernels' nanoseconds per frame-iteration
(event time of LDPC_K_PHYS for the LDS kernel, LDPC_K_PHYS_CN + LDPC_K_PHYS_VN
for the tile kernels, over counter slot 6).  Prints ONE JSON line; --out also
writes it to a file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))

SEED = 20260213


def measure(dec, pg, sig, B, T, steps, **kw):
    import numpy as np
    from ldpc_amd.device import phys_kernel_name
    dec.phys_mc_run(pg, SEED, [sig], B, 0, T, **kw)  # warm-up (builds the layer table)
    dec.profile_read()
    dec.profile(True)
    tot = np.zeros(7, np.int64)
    t0 = time.perf_counter()
    for s in range(steps):
        tot += dec.phys_mc_run(pg, SEED, [sig], B, (s + 1) * B, T, **kw)[0]
    dt = time.perf_counter() - t0
    dec.profile(False)
    prof = dec.profile_read()
    frames, fi = int(tot[0]), max(int(tot[6]), 1)
    lds_ms, cn_ms, vn_ms = prof["phys"][0], prof["phys_cn"][0], prof["phys_vn"][0]
    name = {k: v for k, v in kw.items() if k in ("cn", "schedule", "tile", "hbm")}
    return {"cn": kw["cn"], "schedule": kw["schedule"], "tile_flag": bool(kw.get("tile", False)),
            "kernel": phys_kernel_name(pg, **name), "cw_per_s": frames / dt, "fer": int(tot[1]) / frames,
            "avg_iters": int(tot[6]) / frames, "kernel_ms": lds_ms + cn_ms + vn_ms, "phys_ms": lds_ms,
            "phys_cn_ms": cn_ms, "phys_vn_ms": vn_ms,
            "kernel_ns_per_frame_iteration": (lds_ms + cn_ms + vn_ms) * 1e6 / fi}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--which", choices=("dvbs2", "wimax"), required=True)
    ap.add_argument("--snrs", type=float, nargs="+", default=None,
                    help="default: -2.0 -1.5 1.0 (dvbs2), -2.5 1.0 (wimax)")
    ap.add_argument("--dvbs2-frames", type=int, default=8192, help="frames per step (bench.py config 5: 8192)")
    ap.add_argument("--wimax-frames", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row (after one warm-up)")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mc-stats", type=int, default=None, metavar="MAX_FAILED",
                    help="collect the Monte-Carlo statistics (Decoder.mc_stats) with this many failed-frame records "
                         "per point: the cost of statistics on (default: off)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    import ldpc_amd
    from ldpc_amd import ira
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Decoder, Graph

    if a.which == "dvbs2":
        code, B = "dvbs2_profile_64800_0.5", a.dvbs2_frames
        pg = Graph(ira.dvbs2_profile_matrix(), device=a.device)
        dec = Decoder(pg, B)
        rows = (dict(cn="nms", schedule="flooding"), dict(cn="nms", schedule="layered"))
        snrs = a.snrs or [-2.0, -1.5, 1.0]
    else:
        code, B = "wimax_2304_0.5", a.wimax_frames
        edd = ldpc_amd.load_committed_code(code)
        pg = Graph(edd.physical_matrix(), device=a.device)
        dec = Decoder(Graph(edd._h_std, device=a.device), B)  # frame source = H_std
        rows = (dict(cn="nms", schedule="layered"), dict(cn="nms", schedule="layered", tile=True))
        snrs = a.snrs or [-2.5, 1.0]
    if a.mc_stats is not None:
        dec.mc_stats(True, a.mc_stats)
    points = []
    for snr in snrs:
        sig = mc.sigma_for_snr(snr)
        points.append({"snr_db": snr,
                       "configs": [measure(dec, pg, sig, B, a.iters, a.steps, alpha=a.alpha, **r) for r in rows]})
    dec.close()
    line = json.dumps({"tool": "bench_phys_layered_tile", "which": a.which, "code": code, "frames_per_step": B,
                       "steps": a.steps, "max_iter": a.iters, "alpha": a.alpha, "mc_stats": a.mc_stats, "points": points})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
