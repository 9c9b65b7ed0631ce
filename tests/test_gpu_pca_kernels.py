"""GPU: dh_embed_scatter and dh_embed_project (deephisto_amd/csrc/embed.hip) against tests/helpers/pca_ref.py.

Scatter: D in {64, 128, 192, 512} (a lone diagonal tile, the first mirrored tile, an odd tile count, the ResNet-18 width) x n in {1, 2,
63, 1023, 1024, 1025, 2049, 3100} (one, two, three and four chunks and the ragged row stages), plus (n = 130, D = 2048) and, for the
chunks of one matrix going through the scratch in two batches, (n = 3100, D = 1024); between them the scratch-free walk (one chunk;
two chunks at D = 512) and the batched passes; stand-in features (non-negative with a common mean: the
case that matters) and signed normal rows, every element held to float64 by the gate (m + c + 4) u |t|^T |t|.  Then the order itself,
bit for bit.  Project: D in {64, 512, 2048} x K in {1, 3, 17, 64} x n in {1, 31, 33, 65, 1025} by the gate (D + 4) u.  Worst observed
errors on the MI355X: DESIGN.md section 4.19 (the tests print them per case)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent / "helpers"))
import embed_ref as er  # noqa: E402
import pca_ref as pr  # noqa: E402

pytestmark = pytest.mark.gpu

SCATTER_DS, SCATTER_NS = (64, 128, 192, 512), (1, 2, 63, 1023, 1024, 1025, 2049, 3100)
PROJECT_DS, PROJECT_KS, PROJECT_NS = (64, 512, 2048), (1, 3, 17, 64), (1, 31, 33, 65, 1025)


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


_CACHE: dict = {}


def _rows_of(kind, D, n_max):
    """float32[n_max, D] rows and a float32[D] mean, the same for every test that asks (computed once and never written)."""
    key = (kind, D, n_max)
    if key not in _CACHE:
        if kind == "standin":
            x = er.standin_features(n_max, D, 100 + D)
            mean = x.astype(np.float64).mean(0).astype(np.float32)
        else:
            rng = np.random.default_rng(200 + D)
            x = rng.standard_normal((n_max, D)).astype(np.float32)
            mean = (0.3 * rng.standard_normal(D)).astype(np.float32)
        x.setflags(write=False)
        mean.setflags(write=False)
        _CACHE[key] = (x, mean)
    return _CACHE[key]


def _bits(t):
    return (t.cpu().numpy() if isinstance(t, torch.Tensor) else np.ascontiguousarray(t)).view(np.uint32)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_scatter(dev, x, mean, what):
    from deephisto_amd.pca import centred_scatter
    got = centred_scatter(_t(x, dev), _t(mean, dev)).cpu().numpy()
    want, gate = pr.scatter_ref(x, mean)
    err = np.abs(got.astype(np.float64) - want)
    mag = gate / pr.scatter_coeff(len(x))
    worst = float(np.max(np.divide(err, mag, out=np.zeros_like(err), where=mag > 0)) / pr.U)
    print(f"scatter {what}: worst |S - S64| = {worst:.2f} u |t|^T |t| (gate {pr.scatter_coeff(len(x)) / pr.U:.0f} u)")
    assert np.all(err <= gate), f"{what}: {int((err > gate).sum())} elements past the gate, worst {worst:.2f} u"
    assert np.array_equal(_bits(got), _bits(got.T.copy())), f"{what}: S != S.T"
    return got


# ---- scatter against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SCATTER_NS)
@pytest.mark.parametrize("D", SCATTER_DS)
def test_scatter_against_float64(dev, D, n):
    for kind in ("standin", "normal"):
        x, mean = _rows_of(kind, D, max(SCATTER_NS))
        _check_scatter(dev, x[:n], mean, f"{kind} D={D} n={n}")


@pytest.mark.parametrize("D,n", [(2048, 130), (1024, 3100)])
def test_scatter_against_float64_at_the_wide_shapes(dev, D, n):
    for kind in ("standin", "normal"):
        x, mean = _rows_of(kind, D, n)
        _check_scatter(dev, x, mean, f"{kind} D={D} n={n}")


# ---- bit for bit --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,n", [(128, 2049), (2048, 130), (192, 700), (1024, 3100)])
def test_scatter_repeats_and_ignores_the_stream(dev, D, n):
    from deephisto_amd.pca import centred_scatter
    x, mean = _rows_of("standin", D, max(SCATTER_NS) if D < 1024 else n)
    xd, md = _t(x[:n], dev), _t(mean, dev)
    a = centred_scatter(xd, md)
    b = centred_scatter(xd, md)
    assert np.array_equal(_bits(a), _bits(b)), "two runs agree"
    assert torch.equal(a, a.T)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        c = centred_scatter(xd, md)
    side.synchronize()
    assert np.array_equal(_bits(a), _bits(c)), "a non-default stream gives the same bits"


@pytest.mark.parametrize("D,n", [(128, 2053), (2048, 2053), (1024, 3100)])
def test_scatter_adds_the_chunks_in_ascending_order(dev, D, n):
    """n = 2053: S == fl(fl(S0 + S1) + S2) with the three chunks' own scatter matrices about the same mean, through one batch of
    partials (D = 128) and on the scratch-free walk (D = 2048); n = 3100 at D = 1024: four chunks in two batches."""
    from deephisto_amd.pca import centred_scatter
    x = er.standin_features(n, D, 77)
    mean = _t(x.astype(np.float64).mean(0).astype(np.float32), dev)
    xd = _t(x, dev)
    whole = centred_scatter(xd, mean).cpu().numpy()
    parts = [centred_scatter(xd[lo:lo + 1024], mean).cpu().numpy() for lo in range(0, n, 1024)]
    want = np.zeros_like(parts[0])
    for p in parts:
        want = want + p
    assert want.dtype == np.float32 and np.array_equal(_bits(whole), _bits(want))
    back = np.zeros_like(parts[0])
    for p in parts[::-1]:
        back = back + p
    assert not np.array_equal(_bits(whole), _bits(back)), "the order is observable on these rows"


def test_scatter_chunk_is_one_ascending_chain(dev):
    """D = 64, mean 0, one row with 4096 in column 0 among 1023 rows of ones.  The large row first: S[0][0] starts at 2^24 and every
    later + 1 is lost to rounding, which only ONE chain in ascending row order does.  The large row last: the ones add up exactly to
    1023 and the last step is fl(2^24 + 1023), one rounding of the exact value (the tie 16 778 239 goes to the even 16 778 240)."""
    from deephisto_amd.pca import centred_scatter
    x = np.ones((1024, 64), np.float32)
    x[0, 0] = 4096.0
    zero = torch.zeros(64, dtype=torch.float32, device=dev)
    first = centred_scatter(_t(x, dev), zero).cpu().numpy()
    assert first[0, 0] == 16777216.0
    assert first[0, 1] == first[1, 0] == 4096.0 + 1023.0 and first[1, 1] == 1024.0
    last = centred_scatter(_t(x[::-1], dev), zero).cpu().numpy()
    assert last[0, 0] == np.float32(16777216.0 + 1023.0) == 16778240.0
    assert last[0, 1] == 4096.0 + 1023.0 and last[5, 9] == 1024.0


def test_scatter_is_exact_on_small_integers(dev):
    """Integer rows in 0 .. 15 about an integer mean of 7, n = 3000, D = 192: every product and partial sum is an integer below 2^24,
    so every float32 step is exact and S equals the int64 result bit for bit: no element is dropped, doubled or misplaced."""
    from deephisto_amd.pca import centred_scatter
    n, D = 3000, 192
    xi = np.random.default_rng(9).integers(0, 16, (n, D))
    t = xi - 7
    want = (t.T @ t).astype(np.int64)
    assert int(np.abs(t).max() ** 2) * n < 2 ** 24
    got = centred_scatter(_t(xi.astype(np.float32), dev), torch.full((D,), 7.0, dtype=torch.float32, device=dev)).cpu().numpy()
    assert np.array_equal(got, want.astype(np.float32)) and np.array_equal(got.astype(np.int64), want)


@pytest.mark.parametrize("D,n", [(128, 63), (128, 1029), (2048, 5)])
def test_scatter_never_reads_the_row_behind_n(dev, D, n):
    from deephisto_amd.pca import centred_scatter
    x, mean = _rows_of("normal", D, max(SCATTER_NS) if D != 2048 else 130)
    buf = torch.full((n + 1, D), float("nan"), dtype=torch.float32, device=dev)
    buf[:n] = _t(x[:n], dev)
    got = centred_scatter(buf[:n], _t(mean, dev))
    assert bool(torch.isfinite(got).all())
    assert np.array_equal(_bits(got), _bits(centred_scatter(_t(x[:n], dev), _t(mean, dev))))


def test_scatter_of_no_rows_is_zero(dev, built_lib):
    from deephisto_amd.pca import centred_scatter
    got = centred_scatter(torch.empty((0, 128), dtype=torch.float32, device=dev), torch.ones(128, dtype=torch.float32, device=dev))
    assert tuple(got.shape) == (128, 128) and not bool(got.any())


# ---- project against float64 ----------------------------------------------------------------------------------------------------------
def _comp_of(D, K):
    if ("c", D, K) not in _CACHE:
        rng = np.random.default_rng(17 * D + K)
        c = rng.standard_normal((K, D)).astype(np.float32)
        s = (rng.standard_normal(K) * 3.0).astype(np.float32)
        c.setflags(write=False)
        s.setflags(write=False)
        _CACHE["c", D, K] = (c, s)
    return _CACHE["c", D, K]


@pytest.mark.parametrize("n", PROJECT_NS)
@pytest.mark.parametrize("K", PROJECT_KS)
@pytest.mark.parametrize("D", PROJECT_DS)
def test_project_against_float64(dev, D, K, n):
    from deephisto_amd.pca import project
    comp, scale = _comp_of(D, K)
    scale = scale if K in (3, 64) else None      # NULL (every scale 1) and signed scales
    for kind in ("standin", "normal"):
        x, mean = _rows_of(kind, D, max(PROJECT_NS))
        got = project(_t(x[:n], dev), _t(mean, dev), _t(comp, dev), None if scale is None else _t(scale, dev))
        assert tuple(got.shape) == (n, K) and got.is_contiguous()
        want, gate = pr.project_ref(x[:n], mean, comp, scale)
        err = np.abs(got.cpu().numpy().astype(np.float64) - want)
        worst = float(np.max(np.divide(err, gate, out=np.zeros_like(err), where=gate > 0)) * (D + 4))
        print(f"project {kind} D={D} K={K} n={n}: worst error {worst:.2f} u |s| |t| . |c| (gate {D + 4} u)")
        assert np.all(err <= gate), f"{kind}: worst {worst:.2f} u"


# ---- project, bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 17, 64))
@pytest.mark.parametrize("D", (64, 2048))
def test_project_launch_independence(dev, D, K):
    """Row 40 alone, inside the launch of 1025 and at another place of a shorter launch: the same bits."""
    from deephisto_amd.pca import project
    x, mean = _rows_of("standin", D, max(PROJECT_NS))
    comp, scale = _comp_of(D, K)
    xd, md, cd, sd = _t(x, dev), _t(mean, dev), _t(comp, dev), _t(scale, dev)
    full = project(xd, md, cd, sd)
    alone = project(xd[40:41], md, cd, sd)
    moved = project(xd[7:300], md, cd, sd)
    assert np.array_equal(_bits(alone[0]), _bits(full[40])) and np.array_equal(_bits(moved[33]), _bits(full[40]))
    assert np.array_equal(_bits(moved), _bits(full[7:300]))
    assert np.array_equal(_bits(project(xd, md, cd, sd)), _bits(full)), "a second launch gives the same bits"


def test_project_leaves_the_columns_behind_K(dev):
    from deephisto_amd.pca import project
    D, K, n, ld = 512, 3, 65, 64
    x, mean = _rows_of("standin", D, max(PROJECT_NS))
    comp, _ = _comp_of(D, K)
    xd, md, cd = _t(x[:n], dev), _t(mean, dev), _t(comp, dev)
    out = torch.full((n + 1, ld), -7.25, dtype=torch.float32, device=dev)
    got = project(xd, md, cd, out=out[:n])
    assert got.data_ptr() == out.data_ptr()
    assert bool((out[:n, K:] == -7.25).all()) and bool((out[n] == -7.25).all()), "columns K .. ld - 1 and the row behind n keep their bytes"
    assert np.array_equal(_bits(out[:n, :K].contiguous()), _bits(project(xd, md, cd)))
    wide = project(xd, md, cd, width=ld)
    assert tuple(wide.shape) == (n, ld) and not bool(wide[:, K:].any()) and torch.equal(wide[:, :K], out[:n, :K])


@pytest.mark.parametrize("K", (5, 64))
def test_project_about_zero_is_dh_embed_scores(dev, K):
    from deephisto_amd.embeddings import prototype_scores
    from deephisto_amd.pca import project
    D, n = 512, 333
    x, _ = _rows_of("normal", D, max(PROJECT_NS))
    comp = np.random.default_rng(K).standard_normal((K, D)).astype(np.float32)
    xd, cd = _t(x[:n], dev), _t(comp, dev)
    got = project(xd, torch.zeros(D, dtype=torch.float32, device=dev), cd)
    assert np.array_equal(_bits(got), _bits(prototype_scores(xd, cd, 1.0)))


# ---- refusals by name ------------------------------------------------------------------------------------------------------------------
def test_wrappers_refuse_by_name(dev):
    from deephisto_amd._lib import DeephistoHipError
    from deephisto_amd.pca import centred_scatter, project
    x = torch.zeros((4, 96), dtype=torch.float32, device=dev)
    with pytest.raises(DeephistoHipError, match="D = 96"):
        centred_scatter(x, torch.zeros(96, dtype=torch.float32, device=dev))
    x = torch.zeros((4, 64), dtype=torch.float32, device=dev)
    m = torch.zeros(64, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="mean"):
        centred_scatter(x, torch.zeros(65, dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError, match="GPU memory"):
        centred_scatter(x, torch.zeros(64))
    with pytest.raises(ValueError, match="components"):
        project(x, m, torch.zeros((2, 128), dtype=torch.float32, device=dev))
    with pytest.raises(DeephistoHipError, match="ld = 6"):
        project(x, m, torch.zeros((2, 64), dtype=torch.float32, device=dev), width=6)
    with pytest.raises(ValueError, match="scale"):
        project(x, m, torch.zeros((2, 64), dtype=torch.float32, device=dev), torch.ones(3, dtype=torch.float32, device=dev))
