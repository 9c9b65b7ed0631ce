"""The float64 batch-norm / pooling reference (oracle/bn_ref.py) and the judge of tests/test_gpu_bn_bf16_parity.py (oracle/bn_cases.py), checked
on the CPU against a float32 emulation of the kernels' arithmetic on the very cases and operands the GPU module uses:

  * the emulation -- float32 coefficients, fmas and partial sums in the engine's order of additions, one rounding to bf16 -- passes every
    gate of every case, stays within both caps, and its identical fraction is at least 0.9995, a margin over the 0.999 the kernels are
    asked for (so the floor is one a plain float32 evaluation meets, not one tuned to the kernels);
  * every planted error fails: the projection terms of dz dropped, k1 * 1.02, k2 * 0.98 (the first two move more than 75 % of the
    elements outside the gate), the elements of y below 0.05 scaled by 1.2, the last row left unwritten or stale, the channels of one
    8-channel group swapped, the second instead of the first maximum on a tie, a bits byte with two bits swapped, the join's inner rounding
    skipped.
"""
import numpy as np
import pytest

from oracle import bn_cases as bc
from oracle import bn_ref as br
from oracle.layer_ref import quantum, round_to

HOST_IDENTICAL = 0.9995


def _assert_clean(rep):
    print("\n" + rep.line())
    assert not rep.failures, "\n".join(rep.failures)
    for k, v in rep.figures.items():
        if k.endswith(" identical"):
            assert v >= HOST_IDENTICAL, f"{rep.name}: {k} {v:.5f} under the host margin {HOST_IDENTICAL}"


@pytest.mark.parametrize("name", [c.name for c in bc.BN_CASES])
def test_float32_emulation_passes_bn_case(name):
    c = bc.BN_BY_NAME[name]
    o = bc.bn_operands(name)
    _assert_clean(bc.judge_bn(c, o, bc.emulate_bn(c, o)))


@pytest.mark.parametrize("name", [c.name for c in bc.POOL_CASES])
def test_float32_emulation_passes_pool_case(name):
    c = bc.POOL_BY_NAME[name]
    o = bc.pool_operands(name)
    _assert_clean(bc.judge_pool(c, o, bc.emulate_pool(c, o)))
    _assert_clean(bc.judge_maxpool(c, o, bc.emulate_maxpool(c, o)))


def _planted(name, plant):
    c = bc.BN_BY_NAME[name]
    o = bc.bn_operands(name)
    return bc.judge_bn(c, o, bc.emulate_bn(c, o, plant))


@pytest.mark.parametrize("name", ["r3139_c64", "r16385_c128", "r245_c2048_res_gout"])
@pytest.mark.parametrize("plant,most", [("no_projection", True), ("k1_scaled", True), ("k2_scaled", False)])
def test_planted_backward_coefficient_fails(name, plant, most):
    rep = _planted(name, plant)
    assert any(" dz:" in f for f in rep.failures), rep.line()
    assert not any(" y:" in f for f in rep.failures)
    if most:
        assert rep.figures["dz outside"] > 0.75, rep.line()


@pytest.mark.parametrize("name", ["r3139_c64", "r591_c1024_norelu", "join_r392_c256"])
def test_planted_small_elements_scaled_fails(name):
    rep = _planted(name, "small_scaled")
    assert any(" y:" in f and "outside the gate" in f for f in rep.failures), rep.line()


@pytest.mark.parametrize("name", ["r65_c64", "r16385_c128", "r16388_c512_res_gout"])
@pytest.mark.parametrize("plant", ["last_row_unwritten", "last_row_stale"])
def test_planted_last_row_fails(name, plant):
    rep = _planted(name, plant)
    rows = bc.BN_BY_NAME[name].rows
    assert any(" y:" in f and f"{rows - 1}" in f for f in rep.failures), "\n".join(rep.failures)
    assert any(" dz:" in f for f in rep.failures)


@pytest.mark.parametrize("name", ["r3139_c64", "r245_c2048_res_gout"])
def test_planted_channel_swap_fails(name):
    rep = _planted(name, "swap_channels")
    assert any(" y:" in f and "channels [8, 9, 10" in f for f in rep.failures), "\n".join(rep.failures)


def test_planted_bits_swap_fails():
    rep = _planted("r245_c2048_res_gout", "bits_swapped")
    assert any(" bits:" in f for f in rep.failures) and not any(" y:" in f for f in rep.failures), "\n".join(rep.failures)


def test_planted_join_without_inner_rounding_fails():
    """Within the gate (the inner rounding is half a unit of the branch value) but not the value the two stored roundings define."""
    rep = _planted("join_r392_c256", "join_no_inner_rounding")
    assert any(" y:" in f and "identical" in f for f in rep.failures), rep.line()


@pytest.mark.parametrize("name", ["b2_h16_c64", "b2_h5_c64"])
def test_planted_second_maximum_on_tie_fails(name):
    c = bc.POOL_BY_NAME[name]
    o = bc.pool_operands(name)
    rep = bc.judge_pool(c, o, bc.emulate_pool(c, o, "second_on_tie"))
    assert any("decided windows differ" in f for f in rep.failures), rep.line()
    assert any(" dz:" in f for f in rep.failures)           # the gradient went to the other element
    rep = bc.judge_maxpool(c, o, bc.emulate_maxpool(c, o, "second_on_tie"))
    assert any("windows differ" in f for f in rep.failures) and any(" dx:" in f for f in rep.failures), rep.line()


def test_pool_reference_agrees_with_torch_and_keeps_the_first_maximum():
    import torch
    import torch.nn.functional as F
    x = np.random.default_rng(3).integers(-2, 3, (2, 7, 6, 8)).astype(np.float64)      # few values: ties in most windows
    want, wi = F.max_pool2d(torch.from_numpy(x).permute(0, 3, 1, 2), 3, 2, 1, return_indices=True)
    got, pos = br.pool(x)
    assert np.array_equal(got, want.permute(0, 2, 3, 1).numpy())
    oy, ox = np.arange(got.shape[1])[None, :, None, None], np.arange(got.shape[2])[None, None, :, None]
    flat = (2 * oy + pos.astype(np.int64) // 3 - 1) * x.shape[2] + 2 * ox + pos.astype(np.int64) % 3 - 1
    assert np.array_equal(flat, wi.permute(0, 2, 3, 1).numpy())                       # torch keeps the first maximum too
    d = np.random.default_rng(4).standard_normal(got.shape)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    (F.max_pool2d(xt, 3, 2, 1) * torch.from_numpy(d).permute(0, 3, 1, 2)).sum().backward()
    assert np.allclose(br.pool_scatter(d, pos, 7, 6), xt.grad.permute(0, 2, 3, 1).numpy(), rtol=0, atol=1e-15)


def test_reference_agrees_with_autograd():
    """forward / backward of bn_ref on float64 statistics equal torch autograd of relu(batch_norm(z) + res) in float64."""
    import torch
    rng = np.random.default_rng(5)
    z, res, dy = rng.standard_normal((37, 16)) + 3.0, rng.standard_normal((37, 16)), rng.standard_normal((37, 16))
    gam, bet = rng.random(16) + 0.5, rng.standard_normal(16)
    mu, var = br.column_stats(z)
    inv = 1.0 / np.sqrt(var + br.EPS)
    pre, _ = br.forward(z, gam, bet, mu, inv, res)
    zt, gt, bt = (torch.from_numpy(a).requires_grad_(True) for a in (z, gam, bet))
    y = torch.relu((zt - zt.mean(0)) / torch.sqrt(zt.var(0, unbiased=False) + br.EPS) * gt + bt + torch.from_numpy(res))
    assert np.allclose(np.maximum(pre, 0), y.detach().numpy(), rtol=1e-12, atol=1e-12)
    (y * torch.from_numpy(dy)).sum().backward()
    g = np.where(pre > 0, dy, 0.0)
    s = br.column_grad_sums(z, g, mu, inv)
    assert np.allclose(s["gx"], gt.grad.numpy(), rtol=1e-10, atol=1e-12) and np.allclose(s["g"], bt.grad.numpy(), rtol=1e-10, atol=1e-12)
    dz, _ = br.backward(z, g, gam, mu, inv, s["gx"], s["g"], 37)
    assert np.allclose(dz, zt.grad.numpy(), rtol=1e-9, atol=1e-11)


def test_bits_unsafe_and_zero_unit():
    y = np.array([[0x0000, 0x8000, 0x3F80, 0x0001, 0, 0, 0, 0xBF80]], np.uint16)
    assert br.pack_bits(y).tolist() == [[0b10001100]]
    # 1 + 2^-8 is the midpoint between the bf16 neighbours 1 and 1 + 2^-7
    pre = np.array([1 + 2.0 ** -8, 1 + 2.0 ** -8 + 1e-5, 1e-9, -1e-9, -1.0, 1.25])
    assert br.unsafe(pre, np.full(6, 4.0)).tolist() == [True, False, True, True, False, False]
    assert quantum(0.0, "bf16") == 2.0 ** (-125 - 8) and round_to(0.0, "bf16") == 0.0


def test_float32_lane_sums_explain_the_invstd_miss_at_16384_rows():
    """Why bn2_cs_reduce_kernel adds the lanes of its statistics in double: with the 31 float32 additions of a 512-row group's lanes the
    one-pass variance of a channel whose mean is 8 standard deviations misses the invstd gate (3.72e-6, gate 1e-6; the engine returned
    exactly this before); the same sums with the lanes added in double and rounded once meet it."""
    o = bc.bn_operands("r16384_c128_res_gout")
    n = o.z.shape[0]
    err = {}
    for lanes64 in (False, True):
        mu = bc._colsum32(o.z, True, lanes64) / n
        var = np.maximum(bc._colsum32(o.z * o.z, True, lanes64) / n - mu * mu, 0.0)
        err[lanes64] = float(np.abs(np.sqrt((o.var + 1e-5) / (var + br.EPS)) - 1).max())
    assert err[True] <= 1e-6 < err[False], err


def test_the_four_pixel_pool_case_is_drawn_on_the_reference_alone():
    """b1_h2_c64 takes the first seeded draw whose float64 reference holds no dz element that is pure rounding noise and no window with an
    unsafe element (one of its 64 windows is already over the 1 % cap); draw 0 has such elements."""
    c = bc.POOL_BY_NAME["b1_h2_c64"]
    census = []
    for draw in range(c.draw + 1):
        d = c._replace(draw=draw)
        bc.POOL_BY_NAME[c.name], bc.POOL_CASES[0] = d, d
        bc.pool_operands.cache_clear()
        try:
            census.append(bc.pool_reference_census(d, bc.pool_operands(c.name)))
        finally:
            bc.POOL_BY_NAME[c.name], bc.POOL_CASES[0] = c, c
            bc.pool_operands.cache_clear()
    assert census[-1] == (0, 0) and all(x != (0, 0) for x in census[:-1]), census
