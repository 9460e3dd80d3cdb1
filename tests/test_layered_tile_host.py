"""Host side of the layered schedule's HBM tile path: the flag's value, the
Python options' checks and the command line (no GPU)."""
import pytest

from ldpc_amd import _lib
from ldpc_amd import montecarlo as mc
from ldpc_amd.device import phys_flags


def test_flag_value():
    assert _lib.LDPC_F_LAYERED_TILE == 0x40
    flags = [_lib.LDPC_F_NLLR, _lib.LDPC_F_DEVICE_PTRS, _lib.LDPC_F_STATIC, _lib.LDPC_F_PHYS_HBM, _lib.LDPC_F_SPLIT,
             _lib.LDPC_F_TEST_ZERO, _lib.LDPC_F_LAYERED_TILE]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def test_header_defines_the_same_value():
    import os
    import re
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "ldpc_hip.h")).read()
    assert re.search(r"#define\s+LDPC_F_LAYERED_TILE\s+0x40u\b", text)
    assert re.search(r"#define\s+LDPC_ABI_VERSION\s+5\b", text)


def test_phys_flags():
    assert phys_flags() == 0
    assert phys_flags(tile=True, schedule="layered") == _lib.LDPC_F_LAYERED_TILE
    assert phys_flags(hbm=True) == _lib.LDPC_F_PHYS_HBM
    for schedule in ("flooding", "other"):
        with pytest.raises(ValueError, match="layered"):
            phys_flags(tile=True, schedule=schedule)


def test_cli_layered_tile():
    a = mc.parse_args(["--matrix", "wimax_576_0.5", "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered",
                       "--layered-tile"])
    assert a.layered_tile is True
    a = mc.parse_args(["--matrix", "wimax_576_0.5", "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered"])
    assert a.layered_tile is False
    for argv in (["--matrix", "x", "--layered-tile"],
                 ["--matrix", "x", "--mode", "physical", "--layered-tile"],
                 ["--matrix", "x", "--mode", "physical", "--cn-rule", "nms", "--layered-tile"]):
        with pytest.raises(SystemExit):
            mc.parse_args(argv)


def test_cli_dvbs2_profile(capsys):
    name = "dvbs2_profile_64800_0.5"
    assert name in mc.IRA_CODES
    a = mc.parse_args(["--matrix", name, "--mode", "physical", "--cn-rule", "nms", "--schedule", "layered"])
    assert (a.matrix, a.mode, a.layered_tile) == (name, "physical", False)
    with pytest.raises(SystemExit):
        mc.parse_args(["--matrix", name])
    assert "physical" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        mc.parse_args(["--matrix", name, "--mode", "parity"])


def test_simulate_refuses_before_any_device_call():
    with pytest.raises(ValueError, match="physical"):
        mc.simulate("dvbs2_profile_64800_0.5", [0.0], 4, 5)
    with pytest.raises(ValueError, match="layered"):
        mc.simulate("wimax_576_0.5", [0.0], 4, 5, mode="physical", cn_rule="nms", layered_tile=True)
