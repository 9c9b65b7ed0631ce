"""GPU: every launch path of the 3x3 convolutions gives the PARENT commit's bits (tests/helpers/conv3_paths.py lists the paths and shapes).

For a change to the host side of the convolutions -- the launch plan (csrc/conv3_plan_host.h), the table cache, the kernel dispatch
(csrc/conv3x3_launch.inc) -- that means to leave every launch as it is.  The kernels write every output once and use no atomics, so equality with
the parent library is exact.  No fixture is committed: the parent library is built in the same session (tools/vs_parent.sh builds it from git
and runs this test) and named by DH_PARENT_LIB; without that variable the test cannot run and skips."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]


def _helper(out, lib_path=None):
    cmd = [sys.executable, str(REPO / "tests" / "helpers" / "conv3_paths.py"), str(out)] + ([str(lib_path)] if lib_path else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.skipif(not os.environ.get("DH_PARENT_LIB"), reason="DH_PARENT_LIB: path of the parent commit's libdeephisto_hip.so (tools/vs_parent.sh)")
def test_every_launch_path_gives_the_parent_librarys_bits(built_lib, tmp_path):
    parent = Path(os.environ["DH_PARENT_LIB"])
    assert parent.exists(), parent
    a = _helper(tmp_path / "parent.npz", parent)
    b = _helper(tmp_path / "new.npz")
    assert sorted(a.files) == sorted(b.files) and len(a.files) >= 30
    for k in a.files:
        print(f"{k}: {a[k].shape}")
        assert a[k].shape == b[k].shape and a[k].size > 0
        assert np.array_equal(a[k], b[k]), f"{k}: {int((a[k] != b[k]).sum())} of {a[k].size} elements differ from the parent"
