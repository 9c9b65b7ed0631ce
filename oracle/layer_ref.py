"""float64 reference of ONE convolution + epilogue of the inference engines, and the element-wise gate their stored activations are held to
(tests/test_gpu_layer_parity.py; the reference itself is checked by tests/test_layer_reference_host.py).

A layer is  y = conv(x, w) * scale + shift (+ res) (ReLU)  on operands the caller takes from the engine (bf16- or f32-exact inputs,
weights, scale/shift or folded bias, residual).  `conv_epilogue` evaluates it in float64 (exact up to ~1e-16 relative) and returns

  want = y rounded ONCE, round-to-nearest-even, to the engine's storage type (bf16 or f32);
  A    = conv(|x|, |w|) * |scale| + |shift| + |res|: the magnitude the engine's f32 accumulation error scales with.

The gate (`gate_mask`):  |got - want| <= ulp(want) + gamma_K * A,  gamma_K = K u / (1 - K u), u = 2^-24 (f32 accumulation), where K counts
every f32 rounding between the exact operands and the stored value: cin * ks * ks - 1 additions of the dot product, + 1 per product for
the f32 MFMA (bf16 x bf16 products are exact in f32), + the epilogue's multiply and its one or two additions.  gamma_K * A bounds the
distance between the engine's f32 value y_c and y (Higham, Accuracy and Stability, section 3.1); the final rounding of y_c against that
of y contributes at most one unit of the storage format.  ReLU is 1-Lipschitz, and max-pooling of rounded values equals the pooled
rounding, so the same bound holds after either with A max-pooled alongside.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

MANT = {"bf16": 8, "f32": 24}          # significant bits of the storage format
MIN_EXP = -125                          # frexp exponent of the smallest normal of both formats (2^-126 = 0.5 * 2^-125)


def quantum(v: np.ndarray, fmt: str) -> np.ndarray:
    """ulp of float64 values v in format `fmt` (bf16 / f32): 2^(e - p) for v = m 2^e, 0.5 <= |m| < 1; subnormal spacing below."""
    _, e = np.frexp(np.asarray(v, np.float64))
    return np.ldexp(1.0, np.maximum(e, MIN_EXP) - MANT[fmt])


def round_to(v: np.ndarray, fmt: str) -> np.ndarray:
    """float64 -> the nearest value of `fmt`, ties to even, in ONE rounding (torch's float64 -> bfloat16 cast goes through float32)."""
    v = np.asarray(v, np.float64)
    q = quantum(v, fmt)
    return np.rint(v / q) * q


def conv_epilogue(x, w, scale, shift, stride: int, res=None, relu: bool = True, pool: bool = False, fmt: str = "bf16",
                  exact: bool = False):
    """x [N][cin][H][W], w [cout][cin][ks][ks], scale / shift [cout], res like the output (or None); all taken as float64.
    pool: the fused stem's max-pool 3x3/2/1 after the ReLU.  Returns (want, A) as float64 numpy arrays; exact=True returns the unrounded
    float64 value instead of `want` (the composition test)."""
    d = lambda t: torch.as_tensor(np.asarray(t), dtype=torch.float64)  # noqa: E731
    x, w, sc, sh = d(x), d(w), d(scale)[None, :, None, None], d(shift)[None, :, None, None]
    ks = w.shape[-1]
    y = F.conv2d(x, w, None, stride, ks // 2) * sc + sh
    a = F.conv2d(x.abs(), w.abs(), None, stride, ks // 2) * sc.abs() + sh.abs()
    if res is not None:
        r = d(res)
        y, a = y + r, a + r.abs()
    if relu:
        y = F.relu(y)
    y = y.numpy()
    if not exact:
        y = round_to(y, fmt)
    if pool:
        y = F.max_pool2d(torch.from_numpy(y), 3, 2, 1).numpy()
        a = F.max_pool2d(a, 3, 2, 1)
    return y, a.numpy()


def gamma(K: int) -> float:
    u = 2.0 ** -24
    return K * u / (1 - K * u)


def rounding_count(cin: int, ks: int, fmt: str, res: bool) -> int:
    """K of the gate: the dot product's additions (+ its rounded products in f32), the epilogue's multiply and additions."""
    k = cin * ks * ks
    return (k - 1) + (k if fmt == "f32" else 0) + 2 + (1 if res else 0)


def gate_mask(got, want, A, K: int, fmt: str) -> np.ndarray:
    """True where an element passes |got - want| <= ulp(want) + gamma_K * A."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return np.abs(got - want) <= quantum(want, fmt) + gamma(K) * np.asarray(A, np.float64)


def fold_bn(w, gamma_, beta, mean, var, eps: float = 1e-5):
    """Eval BN folded in float64: (w * s, beta - mean * s), s = gamma / sqrt(var + eps)."""
    f = lambda t: np.asarray(t, np.float64)  # noqa: E731
    s = f(gamma_) / np.sqrt(f(var) + eps)
    return f(w) * s.reshape(-1, *([1] * (np.ndim(w) - 1))), f(beta) - f(mean) * s


def bn_scale_shift(gamma_, beta, mean, var, eps: float = 1e-5):
    """Eval BN as float64 scale / shift (the unfolded engines' epilogue)."""
    f = lambda t: np.asarray(t, np.float64)  # noqa: E731
    s = f(gamma_) / np.sqrt(f(var) + eps)
    return s, f(beta) - f(mean) * s


def topology(model) -> list[dict]:
    """The convs of oracle.resnet18 / oracle.resnet50 in launch order, each with the stored activation it reads (`src`: "input" for the
    stem, else a conv name or "maxpool") and the one it adds (`res`, or None): {name, bn, src, res, stride, relu}."""
    out = [dict(name="conv1", bn="bn1", src="input", res=None, stride=2, relu=True)]
    prev = "maxpool"
    for li in range(1, 5):
        for bi, blk in enumerate(getattr(model, f"layer{li}")):
            pre = f"layer{li}.{bi}"
            chain = [c for c in ("conv1", "conv2", "conv3") if hasattr(blk, c)]
            idt = prev
            src = prev
            for c in chain[:-1]:
                out.append(dict(name=f"{pre}.{c}", bn=f"{pre}.bn{c[-1]}", src=src, res=None, stride=getattr(blk, c).stride[0], relu=True))
                src = f"{pre}.{c}"
            if blk.downsample is not None:
                idt = f"{pre}.downsample.0"
                out.append(dict(name=idt, bn=f"{pre}.downsample.1", src=prev, res=None, stride=blk.downsample[0].stride[0], relu=False))
            last = chain[-1]
            out.append(dict(name=f"{pre}.{last}", bn=f"{pre}.bn{last[-1]}", src=src, res=idt, stride=getattr(blk, last).stride[0], relu=True))
            prev = f"{pre}.{last}"
    return out


def compose(model, x) -> tuple[dict, np.ndarray]:
    """The whole network layer by layer through conv_epilogue in float64 WITHOUT rounding (unfolded eval BN as scale / shift): the stored
    activations by name and the logits of fc(avgpool(last)).  Equals model.double()(x) up to float64 summation order."""
    sd = {k: v.detach().double().numpy() for k, v in model.state_dict().items()}
    acts = {"input": np.asarray(x, np.float64)}
    for L in topology(model):
        sc, sh = bn_scale_shift(sd[L["bn"] + ".weight"], sd[L["bn"] + ".bias"], sd[L["bn"] + ".running_mean"], sd[L["bn"] + ".running_var"])
        acts[L["name"]], _ = conv_epilogue(acts[L["src"]], sd[L["name"] + ".weight"], sc, sh, L["stride"],
                                           acts[L["res"]] if L["res"] else None, L["relu"], exact=True)
        if L["name"] == "conv1":
            acts["maxpool"] = F.max_pool2d(torch.from_numpy(acts["conv1"]), 3, 2, 1).numpy()
    last = acts[topology(model)[-1]["name"]]
    return acts, head(last, sd["fc.weight"], sd["fc.bias"])


def head(last, fc_w, fc_b) -> np.ndarray:
    """float64 fc(avgpool(last)) of a stored activation [N][C][H][W]."""
    return np.asarray(last, np.float64).mean(axis=(2, 3)) @ np.asarray(fc_w, np.float64).T + np.asarray(fc_b, np.float64)
