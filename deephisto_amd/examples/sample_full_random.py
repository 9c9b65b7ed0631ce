"""Random coverage sampling of one slide -- the caller of examples/sample_full_random.py.

The reference's script builds `FullImageRndSampler(img_path, layer=2, patch_size=224, batch_size=16,
mode=INMEMORY_SINGLEPROC)` on a hard-coded `.psi` path and prints the shapes `generator_torch()` yields until every
coverage cell was hit (sample_full_random.py:14-29).  Same loop here; the slide is a path (psimage when installed,
`.npy`), or -- the default -- a closed-form synthetic slide generated in HBM.  The sampler's index logic runs on the
device (coverage map in HBM, rank-space planning on the host) and consumes the global NumPy RNG like the reference.
Prints the patches/s of the iteration at the end.

    python -m deephisto_amd.examples.sample_full_random [--slide PATH] [--side 4096] [--patch 224] [--batch 16] [--seed 0]
"""
from __future__ import annotations

import argparse
import time


def main(argv=None):
    import numpy as np
    import torch

    from .. import tiles
    from ..patch_samplers.full_samplers import FullImageRndSampler, SamplerExecutionMode

    ap = argparse.ArgumentParser()
    ap.add_argument("--slide", default=None, help="slide path (.psi with psimage installed, or .npy); default: synthetic")
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--layer", type=int, default=1)
    ap.add_argument("--patch", type=int, default=224)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--seed", type=int, default=None, help="np.random.seed before sampling (default: unseeded, as the reference)")
    ap.add_argument("--quiet", action="store_true")
    args = ap.parse_args(argv)
    if args.seed is not None:
        np.random.seed(args.seed)
    src = args.slide if args.slide is not None else tiles.synth_slide(args.side, args.side, 0, "cuda")
    patch_sampler = FullImageRndSampler(src, layer=args.layer, patch_size=args.patch, batch_size=args.batch,
                                        mode=SamplerExecutionMode.INMEMORY_SINGLEPROC)
    n, t0 = 0, time.time()
    for inputs, coords, filled_ratio in patch_sampler.generator_torch():
        if not args.quiet:
            print(inputs.shape, coords.shape, filled_ratio)
        n += int(inputs.shape[0])
    torch.cuda.synchronize()
    dt = time.time() - t0
    print(f"{n / dt} items/s")
    return n, dt


if __name__ == "__main__":
    main()
