"""Host side of the fixed-point min-sum decoder's HBM tile path: the new flag
in the header and in the Python layer, and the argument checks of the Python
and command-line interfaces.  No GPU."""
import os
import re

import numpy as np
import pytest

from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from conftest import ROOT

SEED = 20260213


def _header():
    return open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()


def test_flag_value_and_abi_version():
    txt = _header()
    assert re.search(r"^#define\s+LDPC_F_QUANT_TILE\s+0x80u\b", txt, flags=re.M)
    assert re.search(r"^#define\s+LDPC_ABI_VERSION\s+5\b", txt, flags=re.M)
    assert _lib.LDPC_F_QUANT_TILE == 0x80
    # no other flag of the header has that bit
    flags = re.findall(r"^#define\s+(LDPC_F_\w+)\s+(0x[0-9a-fA-F]+)u", txt, flags=re.M)
    others = {name: int(v, 16) for name, v in flags if name != "LDPC_F_QUANT_TILE"}
    assert others and all(v & 0x80 == 0 for v in others.values()), others


def test_phys_flags():
    from ldpc_amd import device
    assert device.phys_flags(qtile=True) == 0x80
    assert device.phys_flags() == 0
    assert device.phys_flags(qtile=True, schedule="layered") == 0x80
    assert device.phys_flags(hbm=True, qtile=True) == _lib.LDPC_F_PHYS_HBM | 0x80
    assert device.phys_flags(tile=True, schedule="layered", qtile=True) == _lib.LDPC_F_LAYERED_TILE | 0x80
    assert device.phys_flags(True, True, "layered") == _lib.LDPC_F_PHYS_HBM | _lib.LDPC_F_LAYERED_TILE  # as before


@pytest.mark.parametrize("cn,schedule", [("nms", "flooding"), ("nms", "layered"), ("oms", "layered"),
                                         ("spa", "flooding")])
def test_qtile_without_qbits_is_a_value_error(cn, schedule):
    """Before it touches the graph or a device (both are None here)."""
    from ldpc_amd import device
    with pytest.raises(ValueError, match="qbits"):
        device.phys_decode(None, np.zeros((1, 7)), 5, cn=cn, schedule=schedule, qtile=True)
    with pytest.raises(ValueError, match="qbits"):
        device.phys_kernel_name(None, cn=cn, schedule=schedule, qtile=True)
    with pytest.raises(ValueError, match="qbits"):
        device.Decoder.phys_mc_run(None, None, SEED, [1.0], 1, 0, 5, cn=cn, schedule=schedule, qtile=True)
    with pytest.raises(ValueError, match="qbits"):
        mc.simulate("wimax_576_0.5", [0.0], 1, 5, mode="physical", cn_rule=cn, schedule=schedule, quant_tile=True)


def test_cli_quant_tile(capsys):
    head = ["--matrix", "x"]
    a = mc.parse_args(head + ["--mode", "physical", "--cn-rule", "nms", "--qbits", "6", "--quant-tile"])
    assert a.quant_tile is True and (a.qbits, a.llr_scale, a.schedule) == (6, 4.0, "flooding")
    a = mc.parse_args(head + ["--mode", "physical", "--cn-rule", "nms", "--schedule", "layered", "--qbits", "6",
                              "--llr-scale", "2", "--quant-tile"])
    assert a.quant_tile is True and (a.schedule, a.llr_scale) == ("layered", 2.0)
    assert mc.parse_args(head + ["--mode", "physical", "--cn-rule", "nms", "--qbits", "6"]).quant_tile is False
    assert mc.parse_args(head).quant_tile is False
    for argv in (["--mode", "physical", "--cn-rule", "nms", "--quant-tile"],   # no --qbits
                 ["--mode", "physical", "--quant-tile"],
                 ["--quant-tile"],                                            # no --mode physical
                 ["--mode", "physical", "--cn-rule", "spa", "--qbits", "6", "--quant-tile"]):  # no fixed-point form
        with pytest.raises(SystemExit) as e:
            mc.parse_args(head + argv)
        assert e.value.code == 2, argv
    capsys.readouterr()
