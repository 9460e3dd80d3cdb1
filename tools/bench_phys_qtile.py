#!/usr/bin/env python3
"""The fixed-point min-sum decoder on the HBM tile kernels, measured on one GPU.

The DVB-S2-profile code (n = 64800, ldpc_amd/ira.py; the graph is its own
frame source), --frames frames per step (bench.py's config 5 uses 8192),
normalized min-sum, on the project's on-device frames, one warm-up and --steps
timed steps per row under ldpc_profile_enable.  Per SNR four rows, same frames:

  fp32   flooding  phys_cn_tile_kernel / phys_vn_tile_kernel   16 B per edge-iteration
  fp32   layered   phys_layer_tile_kernel                       16 B
  q-bit  flooding  phys_qcn_tile_kernel / phys_qvn_tile_kernel   5 B
  q-bit  layered   phys_qlayer_tile_kernel                       6 B

(all chosen automatically: no state of this code fits LDS).  Per row: kernel
name, codewords/s (wall clock of the timed steps), FER, average iterations,
the decode kernels' nanoseconds per frame-iteration (event time of
LDPC_K_PHYS_CN + LDPC_K_PHYS_VN over counter slot 6) and the bytes per second
that time means under the row's bytes-per-edge model (messages and posteriors
only; index loads, Lambda and the syndrome sweeps are not in the model).
Prints ONE JSON line; --out also writes it to a file.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ldpc-simulator_amd"))

SEED = 20260213
# message + posterior bytes per edge and iteration (the tile kernels are HBM-bound)
MODEL_BYTES = {("fp32", "flooding"): 16, ("fp32", "layered"): 16, ("q", "flooding"): 5, ("q", "layered"): 6}


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
    cn_ms, vn_ms = prof["phys_cn"][0], prof["phys_vn"][0]
    assert prof["phys"][1] == 0, "an LDS kernel ran: this tool measures the tile kernels"
    name = {k: v for k, v in kw.items() if k in ("cn", "schedule", "qbits", "llr_scale")}
    fmt = "fp32" if kw.get("qbits") is None else "q"
    bpe = MODEL_BYTES[fmt, kw["schedule"]]
    ns = (cn_ms + vn_ms) * 1e6 / fi
    return {"format": "fp32" if fmt == "fp32" else f"q{kw['qbits']} llr_scale {kw['llr_scale']:g}",
            "schedule": kw["schedule"], "kernel": phys_kernel_name(pg, **name), "cw_per_s": frames / dt,
            "fer": int(tot[1]) / frames, "avg_iters": int(tot[6]) / frames, "kernel_ms": cn_ms + vn_ms,
            "phys_cn_ms": cn_ms, "phys_vn_ms": vn_ms, "count_ms": prof["count"][0],
            "kernel_ns_per_frame_iteration": ns, "model_bytes_per_edge_iteration": bpe,
            "model_GB_per_s": bpe * pg.nnz / ns}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--snrs", type=float, nargs="+", default=[-2.0, -1.5, 1.0])
    ap.add_argument("--frames", type=int, default=8192, help="frames per step (bench.py config 5: 8192)")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=3, help="timed steps per row (after one warm-up)")
    ap.add_argument("--alpha", type=float, default=0.75)
    ap.add_argument("--qbits", type=int, default=6)
    ap.add_argument("--llr-scale", type=float, default=2.0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--mc-stats", type=int, default=None, metavar="MAX_FAILED",
                    help="collect the Monte-Carlo statistics (Decoder.mc_stats) with this many failed-frame records "
                         "per point: the cost of statistics on (default: off)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    a = ap.parse_args(argv)

    from ldpc_amd import ira
    from ldpc_amd import montecarlo as mc
    from ldpc_amd.device import Decoder, Graph

    code, B = "dvbs2_profile_64800_0.5", a.frames
    pg = Graph(ira.dvbs2_profile_matrix(), device=a.device)
    dec = Decoder(pg, B)
    if a.mc_stats is not None:
        dec.mc_stats(True, a.mc_stats)
    q = dict(qbits=a.qbits, llr_scale=a.llr_scale)
    rows = (dict(cn="nms", schedule="flooding"), dict(cn="nms", schedule="layered"),
            dict(cn="nms", schedule="flooding", **q), dict(cn="nms", schedule="layered", **q))
    points = []
    for snr in a.snrs:
        sig = mc.sigma_for_snr(snr)
        points.append({"snr_db": snr,
                       "configs": [measure(dec, pg, sig, B, a.iters, a.steps, alpha=a.alpha, **r) for r in rows]})
    dec.close()
    line = json.dumps({"tool": "bench_phys_qtile", "code": code, "n": pg.n, "edges": pg.nnz, "frames_per_step": B,
                       "steps": a.steps, "max_iter": a.iters, "alpha": a.alpha, "mc_stats": a.mc_stats, "qbits": a.qbits,
                       "llr_scale": a.llr_scale, "points": points})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
