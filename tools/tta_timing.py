"""Cost of test-time augmentation on a 50 000^2 resident slide (the closed-form benchmark slide).

The script itself never opens the GPU: every step is a child process of its own under `timeout`, and a step that fails, faults
or runs out of time ends the run (nothing more is started on the device).

  transform   dh_slide_dihedral, all eight views: HIP events around the call, median of `--reps` after 3 warm-up calls, against
              the bytes a view must move (read h*w*3, write h*w*3): TB/s and the fraction of the 6.3 TB/s copy rate; beside it
              a device copy of the same bytes on the same box, and the torch composition a user has without the kernel
              (`torch.flip(...).contiguous()`, `transpose(0, 1).contiguous()`).  Before anything is timed all eight views of a
              2 048 x 4 099 crop of random bytes are compared with NumPy.
  predict     predict_full_patched (bf16 ResNet-18, 224 / 112) plain, with "flips" and with "d4": wall time, best of 2 after a
              warm-up call, the ratio to the plain run, and the parts that are not forwards: the views' transforms, the origin
              mapping and the folds (HIP events), so that what is left of (augmented - V x plain) is the per-view stream joins.

    python tools/tta_timing.py [--side 50000] [--reps 20] --out profiles/tta_timing.json
"""
from __future__ import annotations

import argparse
import subprocess
import sys
from pathlib import Path

HBM_COPY_TBS = 6.3   # the copy rate DESIGN.md sections 4.7 and 4.14 measure bandwidth fractions against
STEP_LIMIT_S = {"transform": 240, "predict": 420}


def step_transform(args, rows):
    import numpy as np
    import torch
    from _timing import median_ms

    from deephisto_amd import tiles, tta
    dev = torch.device("cuda:0")
    crop_host = np.random.default_rng(0).integers(0, 256, (2048, 4099, 3), dtype=np.uint8)
    crop = torch.from_numpy(crop_host).to(dev)
    for v in range(8):
        want = np.rot90(np.fliplr(crop_host) if v >> 2 else crop_host, v & 3).copy()
        assert torch.equal(tta.dihedral_view(crop, v).cpu(), torch.from_numpy(want)), f"view {tta.VIEWS[v]} differs from NumPy"
    del crop

    side = args.side
    slide = tiles.synth_slide(side, side, 0, dev)
    nbytes = slide.numel()
    out = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    common = dict(side=side, gbytes=round(nbytes / 1e9, 3), reps=args.reps, moved_gbytes=round(2 * nbytes / 1e9, 3))

    def emit(way, med, best, **kw):
        tbs = 2 * nbytes / (med * 1e-3) / 1e12
        rows.emit(way=way, **kw, **common, median_ms=round(med, 3), min_ms=round(best, 3), tb_per_s=round(tbs, 3),
                  of_copy_rate=round(tbs / HBM_COPY_TBS, 3))

    emit("copy", *median_ms(lambda: out.copy_(slide.view(-1)), args.reps))
    for v, name in enumerate(tta.VIEWS):
        emit("dihedral_view", *median_ms(lambda: tta.dihedral_view(slide, v, out=out), args.reps), view=name,
             transposes=bool(v & 1))
    del out
    emit("torch", *median_ms(lambda: torch.flip(slide, (1,)), 5), view="r0f", reps_torch=5)
    emit("torch", *median_ms(lambda: slide.transpose(0, 1).contiguous(), 5), view="r90f", reps_torch=5)


def step_predict(args, rows):
    import torch
    from _timing import best_of, median_ms, whole_slide_case

    from deephisto_amd import tta
    from deephisto_amd.predict import predict_full_patched
    dev = torch.device("cuda:0")
    slide, smp, model = whole_slide_case(dev, side=args.side)
    n, P = smp.n_tiles, smp.patch_size
    common = dict(side=args.side, patch=P, stride=112, n_tiles=n, model="resnet18 bf16")
    plain = best_of(lambda: predict_full_patched(smp, model, 5, downscale=16), 2) * 1e3
    rows.emit(way="predict", tta="off", views=1, **common, wall_ms=round(plain, 2))
    # the parts of an augmented run that are not forwards, one view's worth each
    buf = torch.empty(slide.numel(), dtype=torch.uint8, device=dev)
    o_dev = torch.from_numpy(smp.origins[:n]).to(dev)
    acc, one = torch.zeros((n, 5), device=dev), torch.ones((n, 5), device=dev)
    t_mirror = median_ms(lambda: tta.dihedral_view(slide, "r0f", out=buf), 10)[0]
    t_transpose = median_ms(lambda: tta.dihedral_view(slide, "r90", out=buf), 10)[0]
    t_map = median_ms(lambda: tta.map_origins_device(o_dev, args.side, args.side, P, "r270f"), 10)[0]
    t_fold = median_ms(lambda: acc.add_(one), 10)[0]
    del buf
    for name in ("flips", "d4"):
        aug = tta.TestTimeAugmenter(name)
        info: dict = {}
        wall = best_of(lambda: predict_full_patched(smp, model, 5, downscale=16, tta=aug, tta_info=info), 2) * 1e3
        V = len(aug)
        n_t = sum(v & 1 for v in aug.ids)
        transforms = n_t * t_transpose + (V - 1 - n_t) * t_mirror           # r0 is the slide itself
        rows.emit(way="predict", tta=name, views=V, **common, n_forward_tiles=info["n_forward_tiles"], wall_ms=round(wall, 2),
                  over_plain=round(wall / plain, 3), minus_v_plain_ms=round(wall - V * plain, 2), transforms_ms=round(transforms, 2),
                  map_ms=round(V * t_map, 3), fold_ms=round(V * t_fold, 3))


STEPS = {"transform": step_transform, "predict": step_predict}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step", choices=list(STEPS), default=None, help="run this step in this process (what the driver starts)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")
    if args.step is not None:
        from _timing import Rows
        rows = Rows()
        STEPS[args.step](args, rows)
        rows.write(args.out, mode="a")
        return 0
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("")
    for step, limit in STEP_LIMIT_S.items():
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, __file__, "--step", step, "--side", str(args.side), "--reps",
               str(args.reps)] + (["--out", args.out] if args.out else [])
        rc = subprocess.run(cmd).returncode
        if rc != 0:
            print(f"step {step} ended with status {rc}: nothing more is started", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
