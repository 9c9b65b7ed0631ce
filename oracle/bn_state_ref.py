"""float64 reference of what a training forward of the bf16 engine leaves in its BN running statistics, and of its eval-mode BN, with the
element-wise gates tests/test_gpu_bn_state.py holds them to (self-checked on the CPU by tests/test_bn_state_ref_host.py).

Running statistics.  Every BN of the engine sums the bf16-ROUNDED values of its stored Z (the stem's stem_kernel output, the 3x3 convolutions'
and the 1x1 GEMMs' stored tiles alike: no path takes its sums from accumulators before the rounding), as float32 partial rows
{sum z, sum z^2}; the rows are added in double, mean and variance are formed in double (one-pass form, var = s2 / n - mu^2), cast to
float32, and the update R' = (1 - 0.1f) R + 0.1f stat runs in float32.  Two kernels write it: bn_stat_finalize_onepass_kernel and row
group 0 of bn2_fold_apply_kernel (same arithmetic).  So against float64 on the engine's own Z (n = B Ho Wo rows) and its previous R:

  mean      |R' - (0.9 R + 0.1 mu)|            <= 0.1 gamma(K + 1) mean|z|                   + gamma(4) (0.9 |R| + 0.1 |mu|)
  variance  |R' - (0.9 R + 0.1 var n/(n - 1))| <= 0.1 n/(n - 1) gamma(K + 1) (mean(z^2) + mu^2) + gamma(4) (0.9 |R| + 0.1 var n/(n - 1))

gamma(K + 1): K float32 additions of the longest chain of the producing path (z^2 of a bf16 value is exact in float32, the multiply-add
rounds once) and the cast of the statistic; mean(z^2) + mu^2 is the one-pass form's bound (both of its terms carry the sums' error);
gamma(4): 1 - 0.1f, 0.1f itself against 0.1, the product and the addition of the update.  K per path, read from the kernels as an upper
bound that does not depend on the launch geometry:

  "stats"  bn2_stats_kernel (the stem; any map too large for the channel-sliced kernels): a thread adds at most ceil(n / rpi) rows,
           rpi = 256 / min(C / 8, 256) rows per iteration, then rpi - 1 partial sums across the threads:   K = ceil(n / rpi) + rpi - 1
  "cs"     bn2_cs_reduce_kernel (3x3 convolutions on maps of <= DH_T2_FOLD_ROWS rows): 32 row lanes, each at most ceil(n / 32) rows,
           then 31 additions in index order:                                                               K = ceil(n / 32) + 31
  "gemm"   the 1x1 GEMM's epilogue: one partial row per tile of <= 128 pixels (8 + 15 additions):           K = 128
           (a GEMM whose partial rows do not fit falls back to "cs" / "stats"; at these shapes none does)

Eval route.  bn2_eval_coef_kernel forms scale = gamma / sqrt(rv + eps) and shift = beta - rm scale in double and casts each to float32;
the apply kernels evaluate relu(fma(z, scale, shift) [+ identity]) in float32 and store bf16: every term passes at most 3 roundings
(4 with an identity), and the stored value one bf16 rounding:  |y - want| <= quantum_bf16(want) + gamma(4) (|z scale| + |shift| + |identity|).
At a downsample join the identity is the branch's own BN, rounded to bf16 before the addition (bn2_apply_join_kernel, and the unfused
route through the branch's stored Y alike); its float32 coefficients can move that rounding by one bf16 unit of the identity:
+ quantum_bf16(identity) + gamma(3) (|z2 scale2| + |shift2|).
"""
from __future__ import annotations

import numpy as np

from .layer_ref import gamma, quantum, round_to

MOMENTUM, EPS = 0.1, 1e-5


def chain_length(path: str, n: int, C: int) -> int:
    if path == "stats":
        rpi = 256 // min(C // 8, 256)
        return -(-n // rpi) + rpi - 1
    if path == "cs":
        return -(-n // 32) + 31
    assert path == "gemm"
    return 128


def path_of(name: str, ks: int) -> str:
    """The producing path of conv `name` (kernel size ks) at the maps of the test (all <= 16 384 rows, C a multiple of 64, <= 2048)."""
    return "stats" if name == "conv1" else "gemm" if ks == 1 else "cs"


def running_update_ref(z, run_mean, run_var, K: int):
    """z [n][C] (the engine's stored Z, bf16-exact), previous running statistics [C] -> (mean', gate, var', gate)."""
    z = np.asarray(z, np.float64)
    rm, rv = np.asarray(run_mean, np.float64), np.asarray(run_var, np.float64)
    n = z.shape[0]
    mu = z.mean(axis=0)
    var = ((z - mu) ** 2).mean(axis=0)                      # two-pass in float64: exact to 1e-16 of mean(z^2)
    unb = var * n / (n - 1) if n > 1 else var
    g, gu = gamma(K + 1), gamma(4)
    want_m = (1 - MOMENTUM) * rm + MOMENTUM * mu
    gate_m = MOMENTUM * g * np.abs(z).mean(axis=0) + gu * ((1 - MOMENTUM) * np.abs(rm) + MOMENTUM * np.abs(mu))
    want_v = (1 - MOMENTUM) * rv + MOMENTUM * unb
    fac = n / (n - 1) if n > 1 else 1.0
    gate_v = MOMENTUM * fac * g * ((z * z).mean(axis=0) + mu * mu) + gu * ((1 - MOMENTUM) * np.abs(rv) + MOMENTUM * unb)
    return want_m, gate_m, want_v, gate_v


def running_update_f32(z, run_mean, run_var, tile: int, biased: bool = False, momentum: float = 0.1):
    """The engine's arithmetic restated: float32 sums over tiles of `tile` rows added in index order, the tiles' partial rows added in
    double, the update in float32.  biased / momentum: planted errors the gate has to refuse."""
    F = np.float32
    z = np.asarray(z, F)
    n = z.shape[0]
    s1 = np.zeros(z.shape[1], np.float64)
    s2 = np.zeros(z.shape[1], np.float64)
    for r0 in range(0, n, tile):
        a, b = np.zeros(z.shape[1], F), np.zeros(z.shape[1], F)
        for r in range(r0, min(n, r0 + tile)):
            a = a + z[r]
            b = (z[r].astype(np.float64) ** 2 + b).astype(F)
        s1 += a
        s2 += b
    mu = s1 / n
    var = np.maximum(s2 / n - mu * mu, 0.0)
    unb = var if (biased or n == 1) else var * n / (n - 1)
    m = F(momentum)
    rm = (F(1) - m) * np.asarray(run_mean, F) + m * mu.astype(F)
    rv = (F(1) - m) * np.asarray(run_var, F) + m * unb.astype(F)
    return rm, rv


def eval_coefficients(gamma_, beta, run_mean, run_var):
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    s = f(gamma_) / np.sqrt(f(run_var) + EPS)
    return s, f(beta) - f(run_mean) * s


def eval_y_ref(z, scale, shift, identity=None, relu: bool = True, join=None):
    """z [n][C], float64 coefficients [C]; identity [n][C] (bf16-exact values the engine adds) or None; join = (z2, scale2, shift2): the
    identity is the downsample branch's BN of its own Z, rounded to bf16.  Returns (want rounded once to bf16, gate)."""
    z = np.asarray(z, np.float64)
    y = z * scale + shift
    A = np.abs(z * scale) + np.abs(shift)
    extra = 0.0
    if join is not None:
        z2, s2, h2 = join
        z2 = np.asarray(z2, np.float64)
        identity = round_to(z2 * s2 + h2, "bf16")
        extra = quantum(identity, "bf16") + gamma(3) * (np.abs(z2 * s2) + np.abs(h2))
    if identity is not None:
        identity = np.asarray(identity, np.float64)
        y, A = y + identity, A + np.abs(identity)
    if relu:
        y = np.maximum(y, 0.0)
    want = round_to(y, "bf16")
    return want, quantum(want, "bf16") + gamma(4) * A + extra


def eval_y_f32(z, scale, shift, identity=None, relu: bool = True, join=None):
    """The apply kernels restated in NumPy float32 (coefficients cast from double, one multiply-add, the identity's addition, bf16 store)."""
    F = np.float32
    fma = lambda a, b, c: (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)  # noqa: E731
    v = fma(np.asarray(z, F), np.asarray(scale).astype(F), np.asarray(shift).astype(F))
    if join is not None:
        z2, s2, h2 = join
        identity = round_to(fma(np.asarray(z2, F), np.asarray(s2).astype(F), np.asarray(h2).astype(F)), "bf16").astype(F)
    if identity is not None:
        v = v + np.asarray(identity, F)
    if relu:
        v = np.maximum(v, F(0))
    return round_to(v, "bf16")
