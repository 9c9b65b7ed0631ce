"""CPU: the float64 weight-gradient reference and its two conditions (oracle/wgrad_ref.py) on the conv shapes of tests/test_gpu_step_wgrad.py.

Operands are what a step holds: x a ReLU'd activation (the stem: an image in [0, 1]) and dz a zero-mean gradient, both bf16-exact, so the
products of a float32 evaluation are exact and K = N - 1 is the bf16 engine's count.

  sound      a float32 evaluation of the same operands in three summation orders -- torch's f32 autograd, the images added in reversed
             order, chunks of 64 flat pixels summed separately and then added (the engines' slab scheme) -- passes every element of the
             gate and the relative-L2 condition; so does a float64 evaluation in another order, rounded once.  The f32 engine's count
             K = 2N - 1 is held the same way on operands that are NOT bf16-exact.
  sharp      every planted error fails at least one of the two conditions: the last image dropped, the last output row of dz dropped, the
             last 64 flat pixels dropped, one output pixel counted twice, ky / kx swapped, x shifted by one column, x taken from the
             residual tensor instead of the source, accumulation in bf16 instead of f32.

Measured here (worst over the shapes): torch's f32 autograd reaches 0.060 of the gate (the 3 x 3 map, N = 45) and 4.7e-7 relative L2 (the
stem), the chunked order 0.060 / 2.7e-7; float32 operands under K = 2N - 1: 0.058 / 6.8e-7.  "One output pixel counted twice" on the stem
(N = 11 520) moves dW by 1.1e-2 relative L2 and stays INSIDE the element gate (0.83 of it): only the L2 condition sees it.  Every other
planted error fails both conditions on every shape: 2.5 (bf16 accumulation, stem) .. 4e7 times the gate, relative L2 1.7e-3 .. 1.2.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import wgrad_ref as wr

#        name          B  cin cout ks s  Hi     where the GPU cases reach it
SHAPES = [("stem", 5, 3, 64, 7, 2, 96),       # bf16 / f32 ResNet-18, B = 5, P = 96: N = 11 520
          ("c3_s1", 5, 64, 64, 3, 1, 24),     # layer 1 at 24 x 24
          ("c3_s2", 5, 64, 128, 3, 2, 24),    # layer2.0.conv1: 24 -> 12
          ("c1_ring", 3, 128, 512, 1, 1, 12),  # ResNet-50 layer2.x.conv3: both channel counts multiples of 128, N = 432 = 6.75 steps
          ("c1_s2", 3, 256, 512, 1, 2, 24),   # ResNet-50 layer2.0.downsample.0
          ("c3_3x3", 5, 512, 512, 3, 1, 3)]   # layer 4 at P = 96: N = 45, less than one 64-pixel step
IDS = [s[0] for s in SHAPES]
bf = lambda t: t.bfloat16().float()  # noqa: E731


@functools.lru_cache(maxsize=None)
def _case(name):
    """(x, dz, residual tensor, ks, stride, want, A, N): operands float32 and bf16-exact; the float64 reference, computed once."""
    i = IDS.index(name)
    _, B, cin, cout, ks, s, Hi = SHAPES[i]
    g = torch.Generator().manual_seed(4100 + i)
    Ho = (Hi + 2 * (ks // 2) - ks) // s + 1
    x = bf(torch.rand(B, cin, Hi, Hi, generator=g)) if name == "stem" else bf(F.relu(torch.randn(B, cin, Hi, Hi, generator=g)))
    other = bf(F.relu(torch.randn(B, cin, Hi, Hi, generator=g)))
    dz = bf(torch.randn(B, cout, Ho, Ho, generator=g) * 1e-3)
    want, A = wr.wgrad(x, dz, ks, s)
    return x, dz, other, ks, s, want, A, wr.terms(dz.shape)


def _f32_autograd(x, dz, ks, s):
    return wr._autograd_dw(x.float(), dz.float(), ks, s).numpy()


def _f32_reversed_images(x, dz, ks, s):
    acc = torch.zeros(dz.shape[1], x.shape[1], ks, ks)
    for b in reversed(range(x.shape[0])):
        acc = acc + wr._autograd_dw(x[b:b + 1].float(), dz[b:b + 1].float(), ks, s)
    return acc.numpy()


def _chunked(x, dz, ks, s, dtype=torch.float32, acc_round=None):
    """Chunks of 64 flat pixels (b, oy, ox) summed separately in `dtype`, then added in order; acc_round rounds the running sum."""
    cols = F.unfold(x.to(dtype), ks, 1, ks // 2, s)                       # [B][cin ks ks][Ho Wo]
    cols = cols.permute(0, 2, 1).reshape(-1, cols.shape[1])              # [N][cin ks ks]
    d = dz.to(dtype).permute(0, 2, 3, 1).reshape(-1, dz.shape[1])        # [N][cout]
    acc = torch.zeros(dz.shape[1], cols.shape[1], dtype=dtype)
    for p0 in range(0, d.shape[0], 64):
        acc = acc + d[p0:p0 + 64].T @ cols[p0:p0 + 64]
        if acc_round is not None:
            acc = acc_round(acc)
    return acc.reshape(dz.shape[1], x.shape[1], ks, ks).double().numpy()


@pytest.mark.parametrize("name", IDS)
def test_float32_evaluations_in_three_orders_pass_both_conditions(name):
    x, dz, _, ks, s, want, A, N = _case(name)
    K = wr.rounding_count(N, "bf16")
    assert K == N - 1
    for label, got in (("f32 autograd", _f32_autograd(x, dz, ks, s)), ("reversed images", _f32_reversed_images(x, dz, ks, s)),
                       ("64-pixel chunks", _chunked(x, dz, ks, s)),
                       ("f64, chunked, rounded once", _chunked(x, dz, ks, s, torch.float64).astype(np.float32).astype(np.float64))):
        el, l2ok, worst, l2 = wr.verdict(got, want, A, K)
        print(f"[wgrad host] {name} N={N} {label}: worst |d| / gate {worst:.3f}, rel L2 {l2:.2e}")
        assert el and l2ok, (name, label, worst, l2)


@pytest.mark.parametrize("name", ["stem", "c3_s2", "c1_s2", "c3_3x3"])
def test_float32_operands_meet_the_f32_engine_count(name):
    """Operands that are not bf16-exact: the products round, K = 2N - 1 (the float32 engine)."""
    i = IDS.index(name)
    _, B, cin, cout, ks, s, Hi = SHAPES[i]
    g = torch.Generator().manual_seed(4200 + i)
    Ho = (Hi + 2 * (ks // 2) - ks) // s + 1
    x = F.relu(torch.randn(B, cin, Hi, Hi, generator=g))
    dz = torch.randn(B, cout, Ho, Ho, generator=g) * 1e-3
    want, A = wr.wgrad(x, dz, ks, s)
    K = wr.rounding_count(wr.terms(dz.shape), "f32")
    assert K == 2 * B * Ho * Ho - 1
    for label, got in (("f32 autograd", _f32_autograd(x, dz, ks, s)), ("64-pixel chunks", _chunked(x, dz, ks, s))):
        el, l2ok, worst, l2 = wr.verdict(got, want, A, K)
        print(f"[wgrad host] f32 operands {name} {label}: worst |d| / gate {worst:.3f}, rel L2 {l2:.2e}")
        assert el and l2ok, (name, label, worst, l2)


def _planted(name):
    """{error: the float32 evaluation a kernel with that error would give}."""
    x, dz, other, ks, s, *_ = _case(name)
    ev = lambda x_, dz_: _f32_autograd(x_, dz_, ks, s)  # noqa: E731
    out = {}
    d = dz.clone(); d[-1] = 0
    out["last image dropped"] = ev(x, d)
    d = dz.clone(); d[:, :, -1, :] = 0
    out["last dz row dropped"] = ev(x, d)
    d = dz.permute(0, 2, 3, 1).reshape(-1, dz.shape[1]).clone(); d[-64:] = 0
    out["last 64 flat pixels dropped"] = ev(x, d.reshape(dz.shape[0], dz.shape[2], dz.shape[3], -1).permute(0, 3, 1, 2).contiguous())
    d = dz.clone(); d[dz.shape[0] // 2, :, dz.shape[2] // 2, dz.shape[3] // 3] *= 2
    out["one output pixel counted twice"] = ev(x, d)
    if ks > 1:
        out["ky / kx swapped"] = np.ascontiguousarray(ev(x, dz).transpose(0, 1, 3, 2))
    xs = torch.zeros_like(x); xs[..., 1:] = x[..., :-1]
    out["x shifted by one column"] = ev(xs, dz)
    out["x from the residual tensor"] = ev(other, dz)
    out["accumulation in bf16"] = _chunked(x, dz, ks, s, acc_round=bf)
    return out


@pytest.mark.parametrize("name", IDS)
def test_every_planted_error_fails_a_condition(name):
    _, _, _, _, _, want, A, N = _case(name)
    K = wr.rounding_count(N, "bf16")
    for label, got in _planted(name).items():
        el, l2ok, worst, l2 = wr.verdict(got, want, A, K)
        print(f"[wgrad host] {name} N={N} planted '{label}': worst |d| / gate {worst:.3g} ({'pass' if el else 'FAIL'}), "
              f"rel L2 {l2:.2e} ({'pass' if l2ok else 'FAIL'})")
        assert not (el and l2ok), f"{name}: '{label}' passes both conditions (|d| / gate {worst:.3g}, rel L2 {l2:.2e})"
        if label != "one output pixel counted twice":
            assert not el and not l2ok, f"{name}: '{label}' is expected to fail both conditions"


def test_gate_and_l2_see_different_errors():
    """Why there are two conditions: at N ~ 1e4 one pixel counted twice stays inside the worst-case element bound; the L2 condition
    fails by three orders of magnitude."""
    _, _, _, _, _, want, A, N = _case("stem")
    el, l2ok, worst, l2 = wr.verdict(_planted("stem")["one output pixel counted twice"], want, A, wr.rounding_count(N, "bf16"))
    assert not l2ok and l2 > 100 * wr.REL_L2, l2
    print(f"[wgrad host] stem, one pixel twice: inside the element gate: {el} ({worst:.3f}), rel L2 {l2:.2e}")
