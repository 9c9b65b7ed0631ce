#!/usr/bin/env python3
"""A/B of two builds of libdeephisto_hip.so on the three kernels of the 32 x 64 embedding tile (dh_embed_scores, dh_embed_assign
for K > 16, dh_embed_project), both loaded into ONE process through separate ctypes handles and run on the
same seeded inputs at a slide's size.
    python3 tools/embed_tile_ab.py --parent <parent .so> --new deephisto_amd/libdeephisto_hip.so --out profiles/embed_tile_ab.json
Bits: every output of `--new` equals that of `--parent` bit for bit (exit status 1 otherwise).
Time: `--rounds` rounds, each one `_timing.median_ms` of 20 calls per library, the library that goes first alternating.  The noise
is the parent's own spread (max - min of its round medians); `new` is within it when the median of its round medians exceeds the
parent's by no more than that."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import _timing  # noqa: F401  (puts the repository root on sys.path)
import torch

N, DS = 198916, (512, 2048)
CASES = (("dh_embed_scores", (5, 64)), ("dh_embed_project", (5, 64)), ("dh_embed_assign", (17, 64)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", required=True)
    ap.add_argument("--new", required=True)
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    assert a.rounds >= 5
    libs = {"parent": C.CDLL(str(Path(a.parent).resolve())), "new": C.CDLL(str(Path(a.new).resolve()))}
    assert libs["parent"]._handle != libs["new"]._handle, "one library loaded twice"
    dev = torch.device("cuda:0")
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    gen = torch.Generator(device=dev).manual_seed(0)
    rows, all_equal = [], True
    for D in DS:
        x = torch.randn((N, D), generator=gen, dtype=torch.float32, device=dev)
        p = torch.randn((64, D), generator=gen, dtype=torch.float32, device=dev)
        mean = torch.randn(D, generator=gen, dtype=torch.float32, device=dev)
        scale = torch.rand(64, generator=gen, dtype=torch.float32, device=dev) + 0.5
        px, pp, pm, ps = (C.c_void_p(t.data_ptr()) for t in (x, p, mean, scale))
        for name, ks in CASES:
            for K in ks:
                ld = -(-K // 4) * 4
                outs = {w: [torch.zeros((N, ld if name == "dh_embed_project" else K), dtype=torch.float32, device=dev),
                            torch.zeros(N, dtype=torch.int32, device=dev)] for w in libs}

                def fn(w):
                    o, lab = (C.c_void_p(t.data_ptr()) for t in outs[w])
                    f = getattr(libs[w], name)
                    if name == "dh_embed_scores":
                        rc = f(px, C.c_int64(N), C.c_int32(D), pp, C.c_int32(K), C.c_float(0.125), o, stream)
                    elif name == "dh_embed_project":
                        rc = f(px, C.c_int64(N), C.c_int32(D), pm, pp, C.c_int32(K), ps, o, C.c_int32(ld), stream)
                    else:   # distances into the first N floats of the output
                        rc = f(px, C.c_int64(N), C.c_int32(D), pp, C.c_int32(K), C.c_int32(0), C.c_int32(0), lab, o, stream)
                    assert rc == 0, f"{name} ({w}) returned {rc}"

                for w in libs:
                    fn(w)
                torch.cuda.synchronize(dev)
                equal = all(torch.equal(s.view(torch.int32), t.view(torch.int32)) for s, t in zip(outs["parent"], outs["new"]))
                all_equal &= equal
                med = {w: [] for w in libs}
                for r in range(a.rounds):
                    for w in (("parent", "new") if r % 2 == 0 else ("new", "parent")):
                        med[w].append(_timing.median_ms(lambda: fn(w), a.reps)[0])
                noise = max(med["parent"]) - min(med["parent"])
                excess = statistics.median(med["new"]) - statistics.median(med["parent"])
                rows.append(dict(kernel=name, n=N, D=D, K=K, bits_equal=equal, parent_ms=statistics.median(med["parent"]),
                                 new_ms=statistics.median(med["new"]), parent_range_ms=noise, excess_ms=excess,
                                 within_noise=excess <= noise, parent_rounds_ms=med["parent"], new_rounds_ms=med["new"]))
                print(json.dumps(rows[-1]), flush=True)
        del x
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(dict(device=torch.cuda.get_device_name(dev), rounds=a.rounds, reps=a.reps, cases=rows),
                                          indent=1) + "\n")
    return 0 if all_equal else 1


if __name__ == "__main__":
    sys.exit(main())
