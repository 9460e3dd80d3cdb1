"""The launch schedule of the physical-mode Monte-Carlo runs, pinned.

The decode results cannot see a dropped compaction or a changed poll rule of
the host loops in ldpc_api.cpp; the launch counts per kind of
Decoder.profile_read() can.  They are deterministic: the frames come from a
seed, and the polls read device counters after a stream sync.  Every case is
one phys_mc_run / bitflip_mc_run on the shape of
test_phys_tile.py::test_phys_mc_hbm_counters_equal_lds (two chunks per point,
the second ending in a ragged tile); its launch counts and its seven counters
per point must equal tests/golden/phys_launches.json exactly.  That file is
written by tools/record_phys_launches.py from a library built at the commit
before a change to the host loops (LDPC_HIP_LIB), never from the code under
test."""
import json
import os

import pytest

import ldpc_amd
from conftest import GOLDEN
from ldpc_amd import montecarlo as mc

SEED = 20260213
CODE = "wimax_576_0.5"
CAPACITY, FRAMES, FRAME0, MAX_ITER = 1024, 2000, 64, 50
SNRS = (-3.0, -2.5, 0.0)
KINDS = ("generate", "count", "phys", "phys_cn", "phys_vn")
GOLDEN_FILE = os.path.join(GOLDEN, "phys_launches.json")

NMS6 = dict(cn="nms", qbits=6)
# id: (Decoder method, its options, environment, mc_stats on)
CASES = {
    "spa_flooding_lds": ("phys_mc_run", {}, {}, False),
    "spa_flooding_hbm": ("phys_mc_run", dict(hbm=True), {}, False),
    "spa_flooding_hbm_nocompact": ("phys_mc_run", dict(hbm=True), {"LDPC_PHYS_COMPACT": "0"}, False),
    "nms_flooding_hbm": ("phys_mc_run", dict(cn="nms", hbm=True), {}, False),
    "nms_layered_lds": ("phys_mc_run", dict(cn="nms", schedule="layered"), {}, False),
    "nms_layered_tile": ("phys_mc_run", dict(cn="nms", schedule="layered", tile=True), {}, False),
    "q6_flooding_lds": ("phys_mc_run", dict(NMS6), {}, False),
    "q6_flooding_qtile": ("phys_mc_run", dict(NMS6, qtile=True), {}, False),
    "q6_layered_qtile": ("phys_mc_run", dict(NMS6, schedule="layered", qtile=True), {}, False),
    "spa_flooding_hbm_stats": ("phys_mc_run", dict(hbm=True), {}, True),
    "q6_flooding_qtile_stats": ("phys_mc_run", dict(NMS6, qtile=True), {}, True),
    "nms_layered_tile_stats": ("phys_mc_run", dict(cn="nms", schedule="layered", tile=True), {}, True),
    "q6_layered_qtile_stats": ("phys_mc_run", dict(NMS6, schedule="layered", qtile=True), {}, True),
    "bitflip_sliced": ("bitflip_mc_run", {}, {}, False),
    "bitflip_generic": ("bitflip_mc_run", dict(generic=True), {}, False),
}


def run_case(case_id):
    """{"launches": {kind: n}, "counters": [[7 ints] per point]} of one case, on a fresh decoder."""
    from ldpc_amd.device import Decoder, Graph
    method, options, env, stats = CASES[case_id]
    edd = ldpc_amd.load_committed_code(CODE)
    dec = Decoder(Graph.cached(edd._h_std), CAPACITY)
    gp = Graph.cached(edd.physical_matrix())
    sig = [mc.sigma_for_snr(s) for s in SNRS]
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        if stats:
            dec.mc_stats(True, 8)
        dec.profile(True)
        counters = getattr(dec, method)(gp, SEED, sig, FRAMES, FRAME0, MAX_ITER, **options)
        prof = dec.profile_read()
    finally:
        for k, v in before.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
        dec.close()
    return {"launches": {k: int(prof[k][1]) for k in KINDS}, "counters": counters.tolist()}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN_FILE) as f:
        return json.load(f)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", sorted(CASES))
def test_phys_mc_launch_schedule(gpu_available, recorded, case_id):
    got = run_case(case_id)
    print(case_id, json.dumps(got))
    want = recorded[case_id]
    assert got["launches"] == want["launches"]
    assert got["counters"] == want["counters"]
