"""GPU: training steps of both engines give the PARENT commit's bits, with the side stream on and off (tests/helpers/train_paths.py lists the runs).

For a change to the host side of the training engines -- the shared core (csrc/train_core.inc: conv record, pack table, backward scheduler), the
engines' passes (csrc/train.inc, csrc/train2.inc) -- that means to leave every launch, its stream and its order as they are: the step uses no
atomics and sums in fixed orders, so losses, logits, gradients, fired buckets and updated parameters equal the parent library's exactly.  No
fixture is committed: the parent library is built in the same session (tools/vs_parent.sh builds it from git and runs this test) and named by
DH_PARENT_LIB; without that variable the test cannot run and skips."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests" / "helpers"))


def _helper(out, side, lib_path=None):
    """One child process: its own time limit, its exit status asserted before the next one starts."""
    cmd = [sys.executable, str(REPO / "tests" / "helpers" / "train_paths.py"), str(out)] + ([str(lib_path)] if lib_path else [])
    env = dict(os.environ, DH_T1_SIDE=str(side), DH_T2_SIDE=str(side))
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, f"side={side} lib={lib_path}: exit {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.skipif(not os.environ.get("DH_PARENT_LIB"), reason="DH_PARENT_LIB: path of the parent commit's libdeephisto_hip.so (tools/vs_parent.sh)")
def test_training_steps_give_the_parent_librarys_bits(built_lib, tmp_path):
    from train_paths import MIN_ARRAYS
    parent = Path(os.environ["DH_PARENT_LIB"])
    assert parent.exists(), parent
    for side in (1, 0):
        a = _helper(tmp_path / f"parent_side{side}.npz", side, parent)
        b = _helper(tmp_path / f"new_side{side}.npz", side)
        assert sorted(a.files) == sorted(b.files) and len(a.files) >= MIN_ARRAYS, (len(a.files), len(b.files), MIN_ARRAYS)
        for k in a.files:
            assert a[k].shape == b[k].shape and a[k].size > 0, k
            assert np.array_equal(a[k], b[k]), f"side={side} {k}: {int((a[k] != b[k]).sum())} of {a[k].size} elements differ from the parent"
        print(f"side={side}: {len(a.files)} arrays equal")
