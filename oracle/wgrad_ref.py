"""float64 reference of ONE convolution's weight gradient, and the two conditions the training engines' conv weight gradients are held
to as a step actually computes them (tests/test_gpu_step_wgrad.py; the reference and the conditions themselves are checked on the CPU by
tests/test_wgrad_reference_host.py).

dW[co][ci][ky][kx] = sum over the N = B Ho Wo output pixels of dz[b][co][oy][ox] * x[b][ci][oy s + ky - pad][ox s + kx - pad], on
operands the caller takes from the engine (the conv's stored input and its own dZ, as the weight-gradient kernel read them).  `wgrad`
evaluates it in float64 through torch autograd of conv2d (pad ks // 2) and returns

  want = the exact dW rounded ONCE to float32 (the gradient arena's type);
  A    = wgrad(|x|, |dz|): the magnitude the engine's f32 accumulation error scales with.

Element gate (`gate`):  |got - want| <= quantum(want, "f32") + gamma_K * A,  gamma_K = K u / (1 - K u), u = 2^-24 (oracle/layer_ref.py).
K counts every f32 rounding between the exact operands and the stored value:

  bf16 engine  K = N - 1   bf16 x bf16 products are exact in f32, and ANY order of the N - 1 f32 additions meets Higham's bound
                           (Accuracy and Stability, section 4.2): per-wave accumulators, k-group hand-offs through LDS, slabs and their
                           reduce kernels only choose the order.  The stem reads the f32 image and rounds it to bf16 on its way into
                           LDS: the caller passes the rounded image, so its products are exact too.
  f32 engine   K = 2N - 1  the products round as well (one more rounding per term, fused or not).

Nothing else rounds: the slab reduce kernels (wgrad_reduce_kernel, wgrad_reduce_taps_kernel) multiply every slab value by a mask that is
exactly 1.0 or 0.0 -- exact in f32 -- before adding it; stem_wgrad_reduce_kernel only adds; a single slab is written straight into the
arena.  No scale is applied anywhere between the accumulators and dW (the 1 / B of the mean loss is already in dlogits).

The gate is a worst-case bound: at N ~ 1e4 it admits an error as large as one output pixel counted twice.  The second condition, per
tensor, does not:  ||got - want||_2 <= 1e-5 ||want||_2  (`REL_L2`: TOL of tests/test_gpu_train_kernels.py, which the same kernels meet
through their hooks at N up to 8e5; a float32 evaluation of these sums sits at <= 5e-7).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr

REL_L2 = 1e-5


def _autograd_dw(x: torch.Tensor, dz: torch.Tensor, ks: int, stride: int) -> torch.Tensor:
    w = torch.zeros(dz.shape[1], x.shape[1], ks, ks, dtype=x.dtype, requires_grad=True)
    y = F.conv2d(x, w, None, stride, ks // 2)
    assert y.shape == dz.shape, f"dz is {tuple(dz.shape)}, the conv of {tuple(x.shape)} gives {tuple(y.shape)}"
    return torch.autograd.grad(y, w, dz)[0]


def wgrad(x, dz, ks: int, stride: int, exact: bool = False):
    """x [B][cin][Hi][Wi], dz [B][cout][Ho][Wo], taken as float64.  Returns (want, A) as float64 numpy arrays [cout][cin][ks][ks];
    exact=True returns the unrounded float64 gradient instead of `want`."""
    d = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64)  # noqa: E731
    x, dz = d(x), d(dz)
    dw = _autograd_dw(x, dz, ks, stride).numpy()
    a = _autograd_dw(x.abs(), dz.abs(), ks, stride).numpy()
    return (dw if exact else lr.round_to(dw, "f32")), a


def terms(dz_shape) -> int:
    """N = B Ho Wo: the number of terms of one element of dW."""
    return int(dz_shape[0]) * int(dz_shape[2]) * int(dz_shape[3])


def rounding_count(n_terms: int, fmt: str) -> int:
    """K of the gate for operands of the engine `fmt` ("bf16": exact products; "f32": rounded products)."""
    return (n_terms - 1) + (n_terms if fmt == "f32" else 0)


def gate(want, A, K: int) -> np.ndarray:
    """The admitted |got - want| of every element."""
    return lr.quantum(want, "f32") + lr.gamma(K) * np.asarray(A, np.float64)


def gate_ratio(got, want, A, K: int) -> np.ndarray:
    """|got - want| / gate per element: inside the gate where <= 1."""
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / gate(want, A, K)


def rel_l2(got, want) -> float:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.linalg.norm((got - want).ravel()) / max(np.linalg.norm(want.ravel()), np.finfo(np.float64).tiny))


def verdict(got, want, A, K: int) -> tuple[bool, bool, float, float]:
    """(every element inside the gate, relative L2 <= REL_L2, worst |got - want| / gate, relative L2)."""
    r = gate_ratio(got, want, A, K)
    l2 = rel_l2(got, want)
    return bool((r <= 1.0).all()), l2 <= REL_L2, float(r.max()), l2
