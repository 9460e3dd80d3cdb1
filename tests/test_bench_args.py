"""bench.py's plain / --full split: a plain run asks for nothing beyond the
headline's timed steps, --full restores every extra at its default, and an
extra's own option still selects it alone (the profiling scripts in tools/)."""
import importlib.util
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("ldpc_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _parse(bench, monkeypatch, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_has_no_extras(bench, monkeypatch):
    a = _parse(bench, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    for name, (off, _) in bench.FULL_EXTRAS.items():
        assert getattr(a, name) == off and not getattr(a, name), name


def test_full_restores_every_extra(bench, monkeypatch):
    a = _parse(bench, monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "2", "--full"])
    assert a.full
    assert (a.extra_snr, a.point_snr, a.cpu_seconds, a.phys_steps) == ("2.0,3.0", "3.0", 12.0, 4)
    assert (a.config4_snr, a.config2, a.config5, a.dropin_calls) == ("1.0:0.5:4.0", 1, 1, 20)


def test_own_option_wins_either_way(bench, monkeypatch):
    a = _parse(bench, monkeypatch, ["--phys-steps", "2", "--dump-outputs", "d"])
    assert a.phys_steps == 2 and a.config2 == 0 and a.extra_snr == "" and a.dump_outputs == "d"
    a = _parse(bench, monkeypatch, ["--full", "--phys-steps", "0", "--extra-snr="])
    assert a.phys_steps == 0 and a.extra_snr == "" and a.config2 == 1
