"""Launched by tests/test_gpu_conv3_vs_parent.py in a fresh process per library: every launch path of the 3x3 convolutions once, at the smallest
shapes that reach it, on seeded operands; saves every output to argv[1] (.npz, raw bits).  argv[2], optional: another build of the library to
load instead of the in-tree one -- the parent commit's (tools/vs_parent.sh).

  fwd_*    conv + scale / shift + residual + ReLU through dh_debug_conv_bn_act, float32 and bf16: stride 1 on the first and last row of
           conv_mfma_shapes.SHAPES at the three launch sizes that reach tile variants 0 / 1 / 2; stride 2 for 64 -> 128 at 16 x 16 and
           256 -> 512 at 7 x 7, B = 3
  net_*    logits of the bf16 and float32 ResNet-18 engines and of the bf16 ResNet-50 engine, three tiles of 64 x 64 (channel-blocked layout,
           16-channel planes into the wide stride-2 kernel at the 8-wide map, the 128-pixel stride-2 kernel at the 4- and 2-wide maps)
  dgrad_*  stride-2 data gradients through dh_debug_dgrad_f32 (every map) and dh_debug_conv_bf16(dgrad = 1) (even maps): the stride-2 shapes of
           test_gpu_train_kernels.test_dgrad_paths, plus B = 2 at sides 8 and 14 (one-window kernel on 128-pixel tiles)."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))
sys.path.insert(0, str(REPO / "tests" / "helpers"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deephisto_amd import _lib  # noqa: E402

if __name__ == "__main__" and len(sys.argv) > 2:
    _lib.LIB_PATH = Path(sys.argv[2]).resolve()

import conv_mfma_shapes as cms  # noqa: E402
from deephisto_amd._lib import check, lib  # noqa: E402

# (cin, cout, B, side of dX, joining gradient)
DGRAD = [(64, 128, 2, 32, False), (256, 512, 3, 14, False), (64, 128, 2, 15, False), (128, 256, 3, 7, True), (64, 128, 40, 56, True), (64, 64, 2, 9, False),
         (64, 128, 2, 8, True), (128, 256, 2, 14, True)]


def _bits(t):
    t = t.cpu().contiguous()
    return t.view(torch.int16).numpy() if t.dtype == torch.bfloat16 else t.numpy().view(np.int32)


def forward_convs(dev, saved):
    for bf16 in (True, False):
        tag, dt = ("bf16", torch.bfloat16) if bf16 else ("f32", torch.float32)
        for stride, cin, cout, H, Bs in [(1,) + cms.SHAPES[0], (1,) + cms.SHAPES[-1], (2, 64, 128, 16, (3,)), (2, 256, 512, 7, (3,))]:
            Ho = (H + 2 - 3) // stride + 1
            x, w, sc, sh, _ = cms.operands(cin, cout, H, max(Bs), 11 * cin + H + stride)
            res = torch.randn(max(Bs), Ho, Ho, cout, generator=torch.Generator().manual_seed(cout + H)).bfloat16()
            for B in Bs:
                x_d, r_d = x[:B].to(dev, dt).contiguous(), res[:B].to(dev, dt).contiguous()
                out = torch.empty((B, Ho, Ho, cout), dtype=dt, device=dev)
                check(lib().dh_debug_conv_bn_act(x_d.data_ptr(), w.data_ptr(), sc.data_ptr(), sh.data_ptr(), r_d.data_ptr(), out.data_ptr(), B, H, H, cin, cout,
                                                 3, stride, 1, 1 if bf16 else 0, None), "dh_debug_conv_bn_act")
                saved[f"fwd_{tag}_s{stride}_{cin}_{H}_B{B}"] = _bits(out)


def networks(dev, saved):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from oracle import resnet18 as o18
    from oracle import resnet50 as o50
    x = torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(64)).to(dev)
    for name, ref, arch, dtype in [("r18_bf16", o18, "resnet18", "bf16"), ("r18_f32", o18, "resnet18", "f32"), ("r50_bf16", o50, "resnet50", "bf16")]:
        m = get_model(5, dtype, arch=arch)
        m.load_state_dict(ref.seeded_model(3, 5, perturb_bn=True).state_dict())
        m.to(dev).eval()
        saved[f"net_{name}"] = _bits(m.forward_infer(x))


def data_gradients(dev, saved):
    for cin, cout, B, H, with_res in DGRAD:
        g = torch.Generator().manual_seed(cin + 3 * H + B)
        Ho = (H + 2 - 3) // 2 + 1
        w = (torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev).contiguous()
        dz = torch.randn(B, Ho, Ho, cout, generator=g).bfloat16()
        r = torch.randn(B, H, H, cin, generator=g).bfloat16()
        for bf16 in (False, True):
            if bf16 and H % 2:
                continue   # (odd maps are unreachable in the bf16 engine: dh_debug_conv_bf16 refuses them)
            dt = torch.bfloat16 if bf16 else torch.float32
            dz_d, r_d = dz.to(dev, dt).contiguous(), r.to(dev, dt).contiguous()
            dx = torch.empty((B, H, H, cin), dtype=dt, device=dev)
            rp = r_d.data_ptr() if with_res else None
            if bf16:
                check(lib().dh_debug_conv_bf16(dz_d.data_ptr(), w.data_ptr(), rp, dx.data_ptr(), B, H, H, cin, cout, 3, 2, 1, None), "dh_debug_conv_bf16")
            else:
                check(lib().dh_debug_dgrad_f32(dz_d.data_ptr(), w.data_ptr(), rp, dx.data_ptr(), B, H, H, cin, cout, 3, 2, None), "dh_debug_dgrad_f32")
            saved[f"dgrad_{'bf16' if bf16 else 'f32'}_{cin}_{cout}_B{B}_{H}"] = _bits(dx)


def main():
    dev = torch.device("cuda:0")
    saved = {}
    forward_convs(dev, saved)
    networks(dev, saved)
    data_gradients(dev, saved)
    np.savez(sys.argv[1], **saved)


if __name__ == "__main__":
    main()
