"""GPU: the stride-1 bf16 3x3 convolution on 16x16x32 MFMAs (conv3x3.inc, M16; DH_CONV_MFMA16) on every tile variant.

1. Every variant against float64: one conv + scale / shift (+ residual) (+ ReLU) through dh_debug_conv_bn_act against oracle/layer_ref.py's
   float64 convolution of the same bf16 operands, under the gate of the per-layer parity tests (tests/test_gpu_layer_parity.py):
   |got - want| <= ulp(want) + gamma_K * A for every element, and its floor of elements bit-identical to the once-rounded exact value.
   Shapes: per layer shape the smallest B at which dh_conv3::pick_stride1 (conv3_tables_host.h, min_tiles = 256) takes the variant --
   tiles = ceil(B / images per tile) * tile rows * tile columns * cout / 64 >= 256 for the first candidate that reaches it:

       64 ->  64, 16 x 16: 2 x 16 x 16 (v0, weights resident, two chunks) B = 511;  16 x 16 (v1) B = 256;  2 x 8 x 8 (v2) below
      128 -> 128, 16 x 16: v0 B = 255, v1 B = 128;       8 x 8: the 8-image fit tile (v0) B = 1017, 4 x 8 x 8 (v1) B = 509
      512 -> 512,  8 x  8: the 8-image fit tile (v0) B = 249, v1 B = 125
      256 -> 256, 14 x 14: five 7 x 14 half-images (fit, masked slots; v0) B = 156, 16 x 16 (v1) B = 64
      512 -> 512,  7 x  7: ten images (fit, masked slots; v0) B = 311, five images (fit; v1) B = 156
   and B = 1 for variant 2 (the fallback).  tests/test_conv_mfma16_host.py checks these B against the header without a GPU; here the
   library's own report (dh_debug_last_conv3) is asserted after every launch.  The inputs are random everywhere, border pixels included,
   so a lane that pads where it should not (or the reverse) shows.  Of a large launch the reference is computed on the first and last
   images and those around the first tile-group boundary and the middle of the batch.
2. One layer, every launch size, same bits, at DH_CONV_MFMA16 = 1 and = 0 (fresh processes: the variable is read once):
   tests/helpers/conv_mfma_shapes.py.
3. DH_CONV_MFMA16 = 0 reproduces the parent commit's library bit for bit on those shapes.  No fixture is committed: the parent library is
   built in the same session (tools/vs_parent.sh builds it from git and runs this test) and named by DH_PARENT_LIB; without that
   variable the test cannot run and skips.
"""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from oracle import layer_ref as lr

pytestmark = pytest.mark.gpu

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests" / "helpers"))
import conv_mfma_shapes as cms  # noqa: E402

IDENTICAL = 0.999   # tests/test_gpu_layer_parity.py, bf16
IMGS = {(16, 0): 2, (16, 1): 1, (8, 0): 8, (8, 1): 4, (14, 0): 5, (14, 1): 1, (7, 0): 10, (7, 1): 5}   # images per tile; variant 2: 2
# the layers (cin, cout) that ship on 16x16x32 (conv3_plan_host.h, conv3_mfma16_layer)
MFMA16_LAYERS = {(64, 64), (256, 256), (512, 512)}

CASES = [(cin, cout, H, k, Bs[k]) for cin, cout, H, Bs in cms.SHAPES for k in range(3)]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _select(B, imgs):
    idx = np.r_[0:4, imgs - 1:imgs + 2, B // 2 - 1:B // 2 + 1, B - imgs - 1:B - imgs + 1, B - 2:B]
    return np.unique(idx[(idx >= 0) & (idx < B)])


@pytest.mark.parametrize("cin,cout,H,variant,B", CASES)
def test_every_variant_matches_float64_reference(dev, cin, cout, H, variant, B):
    x, w, sc, sh, res = cms.operands(cin, cout, H, B, 7 * cin + H + variant)
    sel = _select(B, IMGS.get((H, variant), 2))
    xs = x[sel].permute(0, 3, 1, 2).double().numpy()
    rs = res[sel].permute(0, 3, 1, 2).double().numpy()
    for with_res in (False, True):
        for relu in (False, True):
            out, v, m = cms.run(x, w, sc, sh, res if with_res else None, relu, dev)
            assert v == variant, f"B = {B} ran tile variant {v}, meant {variant}"
            assert m == (16 if (cin, cout) in MFMA16_LAYERS else 32), f"{cin}->{cout} ran on {m}x{m} MFMAs"
            got = out[sel].permute(0, 3, 1, 2).double().numpy()
            want, A = lr.conv_epilogue(xs, w.double().numpy(), sc.double().numpy(), sh.double().numpy(), 1, rs if with_res else None, relu, fmt="bf16")
            ok = lr.gate_mask(got, want, A, lr.rounding_count(cin, 3, "bf16", with_res), "bf16")
            frac = float((got == want).mean())
            print(f"\n{cin}->{cout} {H}x{H} v{variant} B={B} res={with_res} relu={relu}: outside the gate {int((~ok).sum())} of {ok.size}, identical {frac:.5f}")
            bad = np.argwhere(~ok)
            assert ok.all(), f"res={with_res} relu={relu}: {len(bad)} of {ok.size} elements outside the gate; first (image, channel, y, x): " \
                             f"{[(int(sel[i]), int(c), int(y), int(xx)) for i, c, y, xx in bad[:8]]}"
            assert frac >= IDENTICAL, f"res={with_res} relu={relu}: only {frac:.5f} of the elements identical to the rounded exact value"


@pytest.mark.parametrize("knob", ["1", "0"])
def test_one_layer_every_launch_size_same_bits(dev, tmp_path, knob):
    out = tmp_path / f"shapes_{knob}.npz"
    env = dict(os.environ, DH_CONV_MFMA16=knob)
    r = subprocess.run([sys.executable, str(REPO / "tests" / "helpers" / "conv_mfma_shapes.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    for cin, cout, H, _ in cms.SHAPES:
        for k in range(3):
            v, m = z[f"shape_{cin}_{H}_{k}"]
            assert v == k and m == (16 if knob == "1" and (cin, cout) in MFMA16_LAYERS else 32), (cin, H, k, int(v), int(m))


def _helper(out, knob, lib_path=None):
    env = dict(os.environ, DH_CONV_MFMA16=knob)
    cmd = [sys.executable, str(REPO / "tests" / "helpers" / "conv_mfma_shapes.py"), str(out)] + ([str(lib_path)] if lib_path else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.skipif(not os.environ.get("DH_PARENT_LIB"), reason="DH_PARENT_LIB: path of the parent commit's libdeephisto_hip.so (tools/vs_parent.sh)")
def test_knob_0_reproduces_the_parent_library(dev, tmp_path):
    parent = Path(os.environ["DH_PARENT_LIB"])
    assert parent.exists(), parent
    a = _helper(tmp_path / "parent.npz", "0", parent)   # (a parent from before the 16x16x32 kernels reads no such variable)
    b = _helper(tmp_path / "knob0.npz", "0")
    for cin, cout, H, _ in cms.SHAPES:
        k = f"out_{cin}_{H}"
        assert a[k].shape == b[k].shape and a[k].size > 0
        assert np.array_equal(a[k], b[k]), f"{cin}->{cout} at {H}x{H}: {int((a[k] != b[k]).sum())} of {a[k].size} elements differ from the parent"
