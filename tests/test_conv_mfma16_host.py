"""Host checks (no GPU) of the 16x16x32 form of the stride-1 bf16 3x3 convolution (conv3x3.inc, M16).

1. Bank census.  tests/host/conv3_m16_census.cpp builds the M16 lane tables (deephisto_amd/csrc/conv3_tables_host.h) of every stride-1 tile
   candidate of every map the engines produce, replays the window reads of all nine taps and counts the conflicts of every ds_read_b128
   over its four 16-lane service groups; it also checks the tables' consistency (read pixel = stored pixel, every pixel stored once, taps
   inside the window).  Required: 0 conflicts for every shape -- with one exception that no dealing can avoid.  The five-image 7 x 7 fit
   tile (variant 1 of 7 x 7 maps, segments 67 pixels apart at pitch 8) holds 245 pixels in 16 tiles of 16; a tile reads without conflicts
   only if no window index mod 8 occurs more than twice in it, and three of the eight classes mod 8 occur 35 times (7 rows x 5 images;
   the other five 28 times: each image lacks one class) > 16 x 2.  The 32x32x16 lanes of that shape have conflicts for the same reason
   (tests/host/conv3_tables_sweep.cpp allows them 8 service groups); here the shape must not have more than the 32x32x16 lanes it
   replaces, counted over the same number of service-group passes per stage; the count is pinned at what deal_m16_columns gives, 324 (against 648).
2. The launch sizes of tests/test_gpu_conv_mfma_shape.py are the smallest at which dh_conv3::pick_stride1 takes each variant.
"""
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
UNAVOIDABLE = "5x7x7/pitch8/fit/v1/map7"

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


def _build(tmp_path, name, extra=()):
    exe = tmp_path / name
    b = subprocess.run(["g++", "-std=c++17", "-O1", "-g", *extra, str(REPO / "tests" / "host" / f"{name}.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-4000:]
    return exe


def test_m16_bank_census_is_zero(tmp_path):
    exe = _build(tmp_path, "conv3_m16_census", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert lines[-1].startswith("OK ") and int(lines[-1].split()[1]) >= 40, r.stdout[-500:]
    new = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("census ")}
    old = {ln.split()[1]: int(ln.split()[2]) for ln in lines if ln.startswith("census32 ")}
    assert UNAVOIDABLE in new and set(new) == set(old)
    # every tile shape the issue names is among them
    for name in ("2x16x16/pitch18/v0/map16", "8x8x8/pitch9/fit/v0/map8", "5x7x14/pitch15/fit/v0/map14", "10x7x7/pitch8/fit/v0/map7",
                 "1x16x32/pitch34/v0/map64", "1x8x64/pitch66/v0/map56", "4x8x8/pitch12/v1/map8", "2x8x8/pitch12/v2/map8"):
        assert name in new, name
    print("\n".join(f"{k}: {v} (32x32x16 lanes: {old[k]})" for k, v in new.items()))
    bad = {k: v for k, v in new.items() if v != 0 and k != UNAVOIDABLE}
    assert not bad, bad
    assert new[UNAVOIDABLE] == 324 and old[UNAVOIDABLE] == 648, (new[UNAVOIDABLE], old[UNAVOIDABLE])   # pinned: a later dealing must not add to it


def test_gpu_test_launch_sizes_are_the_smallest_per_variant(tmp_path):
    sys.path.insert(0, str(REPO / "tests" / "helpers"))
    import ast
    src = (REPO / "tests" / "helpers" / "conv_mfma_shapes.py").read_text()   # (the module itself imports torch and the library)
    shapes = next(ast.literal_eval(n.value) for n in ast.parse(src).body if isinstance(n, ast.Assign) and n.targets[0].id == "SHAPES")
    exe = _build(tmp_path, "pick_stride1_probe")

    def variant(B, H, cout):
        r = subprocess.run([str(exe), str(B), str(H), str(H), str(cout), "256"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        return int(r.stdout.split()[3])

    assert len(shapes) == 6
    for cin, cout, H, Bs in shapes:
        assert [variant(B, H, cout) for B in Bs] == [0, 1, 2], (cin, H, Bs)
        assert variant(Bs[0] - 1, H, cout) == 1 and variant(Bs[1] - 1, H, cout) == 2 and Bs[2] == 1, (cin, H, Bs)
