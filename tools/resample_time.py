"""Cost of a pyramid layer of a 50 000^2 resident slide (the closed-form benchmark slide).

Timed with HIP events around the whole call (median of `--reps` runs after 3 warm-up calls):

  area_resample      factors 2, 4, 16 and 3/2 against the bytes they must move (read h*w*3, write oh*ow*3): TB/s and the fraction
                     of the 6.3 TB/s copy rate
  torch              the same layer by the torch composition a user has without the kernel: avg_pool2d over float32 chunks of
                     rows, rounded half up (integer factors; the same slide, the same script)
  layer_device(2)    PyramidSlide's build as wall time: a device base (one pass), and a host base uploaded in bands (pageable
                     host memory through PCIe: the copy, not the kernel, sets it)
  predict            predict_full_patched (bf16 ResNet-18, 224 / 112) on layer 2: the yardstick

Before anything is timed the kernel is compared with the NumPy restatement on a 2 048 x 4 099 crop (all four factors), and the
torch composition with the kernel on the same crop (factors 2, 4, 16: float32 holds the sums and the power-of-two divisions
exactly, so the rounding rules agree).

    python tools/resample_time.py [--side 50000] [--reps 20] [--no-host] [--no-predict] --out profiles/resample_time.json
"""
from __future__ import annotations

import argparse
import sys
import time
from fractions import Fraction

HBM_COPY_TBS = 6.3   # the copy rate DESIGN.md section 4.7 measures bandwidth fractions against
CHUNK_ROWS = 4096    # source rows per float32 chunk of the torch composition (2.5 GB at 50 000 columns)


def torch_area(slide, L: int, out):
    """Layer L by avg_pool2d on float32 chunks of rows, rounded half up: what a user composes from torch today."""
    import torch
    import torch.nn.functional as F
    oh, ow = out.shape[:2]
    step = CHUNK_ROWS // L * L
    for r0 in range(0, oh * L, step):
        r1 = min(r0 + step, oh * L)
        x = slide[r0:r1, :ow * L].permute(2, 0, 1).unsqueeze(0).to(torch.float32)
        y = torch.floor(F.avg_pool2d(x, L) + 0.5).clamp_(0, 255).to(torch.uint8)
        out[r0 // L:r1 // L] = y[0].permute(1, 2, 0)
    return out


def main():
    import torch
    from _timing import REPO, Rows, median_ms
    sys.path.insert(0, str(REPO / "tests" / "helpers"))
    import resample_ref as R

    from deephisto_amd import tiles
    from deephisto_amd.resample import PyramidSlide, area_resample, resampled_size

    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-host", action="store_true", help="skip the host base (it needs side^2 * 3 bytes of host memory)")
    ap.add_argument("--no-predict", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    dev = torch.device("cuda:0")
    side, rows = args.side, Rows()
    factors = [Fraction(2), Fraction(4), Fraction(16), Fraction(3, 2)]

    crop = tiles.synth_slide(2048, 4099, 0, dev)
    crop_host = crop.cpu().numpy()
    for f in factors:
        got = area_resample(crop, f)
        assert torch.equal(got.cpu(), torch.from_numpy(R.resample(crop_host, f))), f"the kernel differs from the restatement at {f}"
        if f.denominator == 1:
            assert torch.equal(torch_area(crop, int(f), torch.empty_like(got)), got), f"the torch composition differs at {f}"
    del crop, got

    slide = tiles.synth_slide(side, side, 0, dev)
    nbytes = slide.numel()
    common = dict(side=side, gbytes=round(nbytes / 1e9, 3))
    for f in factors:
        oh, ow = resampled_size(side, side, f)
        out = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
        moved = nbytes + out.numel()
        med, best = median_ms(lambda: area_resample(slide, f, out=out), args.reps)
        tbs = moved / (med * 1e-3) / 1e12
        row = dict(way="area_resample", factor=str(f), **common, reps=args.reps, median_ms=round(med, 3), min_ms=round(best, 3),
                   moved_gbytes=round(moved / 1e9, 3), tb_per_s=round(tbs, 3), of_copy_rate=round(tbs / HBM_COPY_TBS, 3))
        if f.denominator == 1:
            tmed, tbest = median_ms(lambda: torch_area(slide, int(f), out), args.reps)
            row.update(torch_median_ms=round(tmed, 3), torch_min_ms=round(tbest, 3), torch_over_kernel=round(tmed / med, 2))
        rows.emit(**row)
        del out
        torch.cuda.empty_cache()

    def wall(fn, reps=5):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        return sorted(t)[reps // 2] * 1e3

    row = dict(way="layer_device", layer=2, **common,
               device_base_wall_ms=round(wall(lambda: PyramidSlide(slide).layer_device(2)), 3))
    layer2 = PyramidSlide(slide).layer_device(2)
    if not args.no_host:
        host = slide.cpu().numpy()
        p = PyramidSlide(host, device=dev)
        assert torch.equal(p.layer_device(2), layer2), "the banded build differs from the one-pass build"
        row.update(host_base_wall_ms=round(wall(lambda: PyramidSlide(host, device=dev).layer_device(2), 3), 1),
                   host_band_rows=p.band_rows(2), host_bands=-(-(side // 2 * 2) // p.band_rows(2)))
        row["host_gb_per_s"] = round(nbytes / 1e9 / (row["host_base_wall_ms"] * 1e-3), 2)
        del host, p
    del slide
    torch.cuda.empty_cache()
    if not args.no_predict:
        from deephisto_amd.examples.predict_full_patched import predict_full_patched
        from deephisto_amd.models.patch_cls_simple.model import get_model
        from deephisto_amd.patch_samplers.full_samplers import FullImageDenseSampler
        smp = FullImageDenseSampler(layer2, layer=2, patch_size=224, batch_size=64, stride=112, device=dev)
        torch.manual_seed(0)
        model = get_model(5, "bf16", arch="resnet18").to(dev).eval()
        t = []
        for _ in range(3):   # the first round is the warm-up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            predict_full_patched(smp, model, 5, downscale=16)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        row.update(predict_layer2_ms=round(min(t[1:]) * 1e3, 2),
                   device_build_of_predict=round(row["device_base_wall_ms"] / (min(t[1:]) * 1e3), 4))
        if "host_base_wall_ms" in row:
            row["host_build_of_predict"] = round(row["host_base_wall_ms"] / (min(t[1:]) * 1e3), 4)
    rows.emit(**row)
    rows.write(args.out)


if __name__ == "__main__":
    main()
