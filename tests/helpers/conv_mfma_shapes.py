"""Launched by tests/test_gpu_conv_mfma_shape.py in a fresh process (the library reads DH_CONV_MFMA16 once): every stride-1 bf16 3x3 layer shape
of the test at the three launch sizes that reach tile variants 0 / 1 / 2, through dh_debug_conv_bn_act with a residual and ReLU.  Asserts that the
images shared by the three launches are bit-equal, and saves to argv[1] (.npz) the first and last shared images of each shape plus the
(variant, MFMA shape) of each launch as the library reports them (absent in a library without dh_debug_last_conv3).
argv[2], optional: another build of the library to load instead of the in-tree one, e.g. the parent commit's
(tests/test_gpu_conv_mfma_shape.py::test_knob_0_reproduces_the_parent_library, tools/vs_parent.sh)."""
import ctypes as C
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deephisto_amd import _lib  # noqa: E402
from deephisto_amd._lib import check, lib  # noqa: E402

if __name__ == "__main__" and len(sys.argv) > 2:
    _lib.LIB_PATH = Path(sys.argv[2]).resolve()
    if not hasattr(C.CDLL(str(_lib.LIB_PATH)), "dh_debug_last_conv3"):   # a build from before the getter
        _lib.DEBUG_SIGNATURES.pop("dh_debug_last_conv3")

# (cin, cout, H, B of variant 0 / 1 / 2): the smallest B at which dh_conv3::pick_stride1 takes the variant (tests/test_gpu_conv_mfma_shape.py)
SHAPES = [(64, 64, 16, (511, 256, 1)), (128, 128, 16, (255, 128, 1)), (128, 128, 8, (1017, 509, 1)), (512, 512, 8, (249, 125, 1)),
          (256, 256, 14, (156, 64, 1)), (512, 512, 7, (311, 156, 1))]


def operands(cin, cout, H, B, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, H, cin, generator=g).bfloat16()          # NHWC; the border pixels are as random as the rest
    w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).bfloat16().float().contiguous()
    sc = (0.5 + torch.rand(cout, generator=g)).contiguous()
    sh = (0.2 * torch.randn(cout, generator=g)).contiguous()
    res = torch.randn(B, H, H, cout, generator=g).bfloat16()
    return x, w, sc, sh, res


def run(x, w, sc, sh, res, relu, dev):
    """-> (out [B][H][W][cout] bf16 on the host, variant, mfma); variant / mfma None without the getter"""
    B, H, _, cin = x.shape
    cout = w.shape[0]
    x_d = x.to(dev).contiguous()
    r_d = res.to(dev).contiguous() if res is not None else None
    out = torch.empty((B, H, H, cout), dtype=torch.bfloat16, device=dev)
    check(lib().dh_debug_conv_bn_act(x_d.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), r_d.data_ptr() if r_d is not None else None,
                                     out.data_ptr(), B, H, H, cin, cout, 3, 1, 1 if relu else 0, 1, None), "dh_debug_conv_bn_act")
    v, m = C.c_int32(-2), C.c_int32(-2)
    if "dh_debug_last_conv3" in _lib.DEBUG_SIGNATURES:
        check(lib().dh_debug_last_conv3(C.byref(v), C.byref(m)), "dh_debug_last_conv3")
        return out.cpu(), v.value, m.value
    return out.cpu(), None, None


def main():
    dev = torch.device("cuda:0")
    saved = {}
    for cin, cout, H, Bs in SHAPES:
        x, w, sc, sh, res = operands(cin, cout, H, Bs[0], cin * 100 + H)
        outs = []
        for k, B in enumerate(Bs):
            o, v, m = run(x[:B], w, sc, sh, res[:B], True, dev)
            if v is not None and len(sys.argv) <= 2:   # (another build's report is not under test)
                assert v == k, f"{cin}->{cout} at {H}x{H}, B = {B}: variant {v}, meant {k}"
                saved[f"shape_{cin}_{H}_{k}"] = np.array([v, m])
            outs.append(o.view(torch.int16).numpy())
        for k in (1, 2):
            assert np.array_equal(outs[0][:Bs[k]], outs[k]), f"{cin}->{cout} at {H}x{H}: variant {k} (B = {Bs[k]}) differs from variant 0 on the shared images"
        saved[f"out_{cin}_{H}"] = np.concatenate([outs[0][:2], outs[0][-2:]])
    np.savez(sys.argv[1], **saved)


if __name__ == "__main__":
    main()
