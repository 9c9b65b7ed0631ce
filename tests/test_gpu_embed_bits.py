"""GPU: the bits of the 32 x 64 tile of deephisto_amd/csrc/embed.hip (dh_embed_scores, dh_embed_assign for K > 16, dh_embed_project)
against tests/golden/embed_tile_bits.npz, recorded on an MI355X from the library before the three kernels shared one tile
(tools/embed_bits.py --help has the recipe).  The float64 gates and cross-kernel equalities of the other embed tests would not
notice the three kernels changing their summation order together; this does.  Cases and inputs: tests/helpers/embed_bits_cases.py."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import embed_bits_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "embed_tile_bits.npz"


@pytest.fixture(scope="module")
def recorded():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def computed(built_lib):
    assert torch.cuda.is_available()
    return cases.run(built_lib, torch, torch.device("cuda:0"))


def test_every_recorded_array_bit_for_bit(recorded, computed):
    assert sorted(recorded) == sorted(computed)
    for name, want in recorded.items():
        got = computed[name]
        assert got.dtype == want.dtype and got.shape == want.shape, name
        if name.startswith("assign_label"):
            assert np.array_equal(got, want), f"{name}: {int((got != want).sum())} labels differ"
        else:
            differ = got.view(np.uint32) != want.view(np.uint32)
            assert not differ.any(), f"{name}: {int(differ.sum())} of {differ.size} elements differ"


def test_what_the_fixture_exercises(recorded):
    """The recorded cases are the ones meant: the columns behind K untouched, both assignment passes won somewhere, and a
    summation order that shows -- the scores are not the float64 product rounded once."""
    for D in cases.DS:
        x, p = cases.inputs(D)[:2]
        differ = 0
        for K in cases.SCORE_KS:
            out = recorded[f"project_D{D}_K{K}"]
            assert out.shape == (cases.N, cases.ld_of(K)) and np.all(out[:, K:] == cases.SENTINEL) and np.all(out[:, :K] != cases.SENTINEL)
            want = np.float32(x.astype(np.float64) @ p[:K].T.astype(np.float64) * cases.SCORE_SCALE)
            differ += int((recorded[f"scores_D{D}_K{K}"].view(np.uint32) != want.view(np.uint32)).sum())
        assert differ > 0, "the order of the chain cannot be seen on these inputs"
        merged = recorded[f"assign_label_D{D}_Kmerge"]
        assert merged.min() >= 0 and (merged < 64).any() and (merged >= 64).any() and merged.max() < 64 + 17
        for K in cases.ASSIGN_KS:
            lab = recorded[f"assign_label_D{D}_K{K}"]
            assert lab.min() >= 0 and lab.max() < K
