"""Fork safety of the drop-in (GPU).  Named to run FIRST in the GPU session:
main.py's parent never starts HIP before it forks, and neither may this
process before fork_dropin.run() (it checks); where an earlier test of the
session has started it, run() is replayed in a fresh process instead.  See
tests/fork_dropin.py."""
import os
import subprocess
import sys

import pytest

import fork_dropin
from ldpc_amd import _lib


@pytest.mark.gpu
def test_main_py_threads_pattern_bit_exact():
    """Parent builds SPA_Decoder (main.py:221), 2 forked workers build their own
    and decode the reference's golden frames (main.py:78, :248-256): bit-exact."""
    if _lib.hip_started_here():
        # an earlier test started HIP here (the whole suite in one session: tests/test_abi.py asks for
        # the device count): the same run() in a fresh process that has not
        r = subprocess.run([sys.executable, "-c", "import fork_dropin as f; b, p = f.run(workers=2, frames=16); "
                            "print('FORK', [str(i) for i in b], len(p))"],
                           cwd=os.path.dirname(os.path.abspath(__file__)), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out = [ln for ln in r.stdout.splitlines() if ln.startswith("FORK ")][-1]
        assert out.startswith("FORK [] "), f"frames differing from the reference: {out}"
        assert int(out.rsplit(" ", 1)[1]) >= 1
        return
    bad, pids = fork_dropin.run(workers=2, frames=16)
    assert bad == [], f"frames differing from the reference: {bad}"
    assert len(pids) >= 1


@pytest.mark.gpu
def test_child_forked_after_hip_refuses():
    """A child forked after its parent started HIP gets LdpcError, not a hang."""
    assert fork_dropin.run_poisoned() == "refused"
