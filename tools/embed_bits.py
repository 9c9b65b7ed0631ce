#!/usr/bin/env python3
"""Record tests/golden/embed_tile_bits.npz: the bits of dh_embed_scores, dh_embed_assign and dh_embed_project on the cases of
tests/helpers/embed_bits_cases.py, from one library loaded with ctypes (not through deephisto_amd._lib, so any build will do).

The fixture pins the arithmetic order of the 32 x 64 tile of deephisto_amd/csrc/embed.hip.  It was recorded on an MI355X from the
library of the commit BEFORE the three tile kernels were folded into sc_tile:
    git worktree add --detach /tmp/parent <that commit> && (cd /tmp/parent && python3 -m deephisto_amd.build)
    python3 tools/embed_bits.py --lib /tmp/parent/deephisto_amd/libdeephisto_hip.so --out tests/golden/embed_tile_bits.npz
Re-record it only when the arithmetic is meant to change, from the library that is to become the reference;
tests/test_gpu_embed_bits.py then holds every later library to those bits.  `--check` reads a fixture back without a GPU and
reports its size and whether the summation order is observable in it (the scores differ somewhere from the float64 product
rounded once)."""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

REPO = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(REPO / "tests" / "helpers"))
import embed_bits_cases as cases  # noqa: E402


def order_observable(arrays) -> int:
    """How many recorded scores differ from np.float32(x @ p.T * scale) computed in float64."""
    differ = 0
    for D in cases.DS:
        x, p = cases.inputs(D)[:2]
        for K in cases.SCORE_KS:
            want = np.float32(x.astype(np.float64) @ p[:K].T.astype(np.float64) * cases.SCORE_SCALE)
            differ += int((arrays[f"scores_D{D}_K{K}"].view(np.uint32) != want.view(np.uint32)).sum())
    return differ


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the libdeephisto_hip.so to record from")
    ap.add_argument("--out", help="the .npz to write")
    ap.add_argument("--check", help="an .npz to read back instead (no GPU)")
    a = ap.parse_args()
    if a.check:
        with np.load(a.check) as z:
            arrays = {k: z[k] for k in z.files}
        print(f"{a.check}: {len(arrays)} arrays, {Path(a.check).stat().st_size} bytes, "
              f"{order_observable(arrays)} scores differ from the float64 product rounded once")
        return 0 if order_observable(arrays) else 1
    if not a.lib or not a.out:
        ap.error("--lib and --out (or --check)")
    import torch
    lib = C.CDLL(str(Path(a.lib).resolve()))
    arrays = cases.run(lib, torch, torch.device("cuda:0"))
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(a.out, **arrays)
    print(f"{a.out}: {len(arrays)} arrays from {a.lib}, {order_observable(arrays)} scores differ from the float64 product")
    return 0


if __name__ == "__main__":
    sys.exit(main())
