"""Slide, weights, geometry, backbone and output folder of the predict CLI.

The reference hard-codes the slide path, `./output/best_model.pth`, layer 2, downscale 16, patch 224, batch 64 and
(dense branch, :165-167) stride 112; those are the defaults of the flags below.
`--synthetic H W` runs on a closed-form slide when no .psi file / psimage is at hand; `--weights ''` = random init.
`--arch auto` reads the backbone from the checkpoint (ResNet-50 when it has `layer1.0.conv3.weight`)."""
from ..models.patch_cls_simple.model import ARCHS


def add_flags(ap) -> None:
    ap.add_argument("--image", default="/home/xubiker/dev/PATH-DT-MSU.WSS2/images/test/test_01.psi")
    ap.add_argument("--synthetic", type=int, nargs=2, metavar=("H", "W"), default=None)
    ap.add_argument("--weights", default="./output/best_model.pth")
    ap.add_argument("--layer", type=int, default=2)
    ap.add_argument("--downscale_vis", type=int, default=16)
    ap.add_argument("--patch_size", type=int, default=224)
    ap.add_argument("--batch_size", type=int, default=64)
    ap.add_argument("--stride", type=int, default=112)
    ap.add_argument("--random_sampler", action="store_true", default=False)
    ap.add_argument("--ondisk", action="store_true", help="SamplerExecutionMode.ONDISK_MULTIPROC: stream row strips")
    ap.add_argument("--compute_dtype", choices=["f32", "bf16"], default="f32")
    ap.add_argument("--arch", choices=["auto", *ARCHS], default="auto",
                    help="backbone; auto: from the checkpoint's keys (ResNet-18 with --weights ''); ResNet-50 is bf16")
    ap.add_argument("--out_dir", default="./output/")
    ap.add_argument("--no_visualizations", action="store_true")
