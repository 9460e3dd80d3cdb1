"""bench.py --dump-outputs: a plain run at a tiny shape writes the last timed
step's counters, equal to the same mc_run call made here, and its line holds
the headline's keys and none of the --full extras."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, hstd_for

pytestmark = pytest.mark.gpu

SEED = 20260213  # bench.py SEED
FRAMES, STEPS, WARMUP = 64, 2, 1


def test_plain_run_dumps_last_step_counters(gpu_available, tmp_path):
    from ldpc_amd.device import Decoder, Graph
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--frames", str(FRAMES), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(FRAMES / (line["ms_per_step"] / 1e3))
    assert line["unit"] == "codewords/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    for key in ("snr_points", "physical", "config2", "config4", "config5", "dropin"):
        assert key not in line
    assert line["cpu_baseline"] is None
    assert sorted(os.listdir(out)) == ["counters.npy"]
    got = np.load(out / "counters.npy")
    assert got.dtype == np.float64 and got.shape == (1, 7)
    # the last timed step: global frames [(WARMUP + STEPS - 1) * FRAMES, +FRAMES) at the headline's 1 dB
    dec = Decoder(Graph.cached(hstd_for("wimax_2304_0.5")), FRAMES)
    want = dec.mc_run(SEED,[1.0 / math.sqrt(2.0 * 10.0 ** 0.1)], FRAMES, (WARMUP + STEPS - 1) * FRAMES,
                      50, static=True)
    dec.close()
    assert got[0, 0] == FRAMES
    np.testing.assert_array_equal(got, want.astype(np.float64))
