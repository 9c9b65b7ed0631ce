"""float64 references and gates of the training step's tail kernels that are not convolutions: the classifier head (global average pool,
fc forward, fc weight / bias gradient, average-pool + fc data gradient), the cross-entropy loss, and the bf16 gradient wire format
(tests/test_gpu_head.py; checked on the CPU by tests/test_head_ref_host.py).

Gates follow oracle/layer_ref.py: |got - want| <= gamma(K) A (+ one unit of the storage format where the result is stored narrower than
float32), want = the float64 value of the same expression on the same operands, K = the float32 roundings any term passes on its way
into the stored value, A = the sum of the magnitudes of the terms.  K and A are read from the kernels (csrc/train_core_kernels.inc, train_kernels.inc, train2_kernels.inc):

  pooled[b][c] = (sum_q x[b][q][c]) / HW       HW - 1 additions + the division                      K = HW        A = mean_q |x|
  logits[b][k] = sum_c pooled w + bias          per lane C / 64 multiply-adds (one rounding each), 6 butterfly additions, + bias:
                                                C / 64 + 7 <= C for C >= 8                           K = C         A = sum |pooled w| + |bias|
  dW[k][c]     = sum_b dl[b][k] pooled[b][c]    B multiply-adds                                      K = B         A = sum |dl pooled|
  db[k]        = sum_b dl[b][k]                 B additions (the first one to 0 is exact)            K = B         A = sum |dl|
  dX[b][q][c]  = (sum_k dl[b][k] w[k][c]) / HW  n_cls multiply-adds and the division by HW           K = n_cls + 1 A = sum |dl w| / HW
                                                (the division is a rounding of its own unless HW is a power of two); the bf16 engine then
                                                stores bf16: + one bf16 unit of the result.
"""
from __future__ import annotations

import numpy as np

from .layer_ref import gamma, quantum, round_to

U = 2.0 ** -24
EPS_EXPF = 2.0 ** -22      # relative error allowed to the device's expf: 2 ulp (math libraries document 1 to 2 ulp for expf)
EPS_LOGF = 2.0 ** -23      # ... and to logf: 1 ulp


def f64(a):
    return np.asarray(a, np.float64)


# ---- classifier head -------------------------------------------------------------------------------------------------------------------

def pooled_ref(x):
    """x [B][HW][C] -> (want [B][C], gate)."""
    x = f64(x)
    HW = x.shape[1]
    return x.mean(axis=1), gamma(HW) * np.abs(x).mean(axis=1)


def logits_ref(pooled, w, bias):
    """pooled [B][C] (the float32 values the fc kernel read), w [n_cls][C], bias [n_cls] -> (want [B][n_cls], gate)."""
    pooled, w, bias = f64(pooled), f64(w), f64(bias)
    C = pooled.shape[1]
    return pooled @ w.T + bias, gamma(C) * (np.abs(pooled) @ np.abs(w).T + np.abs(bias))


def fc_wgrad_ref(dl, pooled):
    """dl [B][n_cls], pooled [B][C] -> (dW [n_cls][C], gate, db [n_cls], gate)."""
    dl, pooled = f64(dl), f64(pooled)
    B = dl.shape[0]
    return dl.T @ pooled, gamma(B) * (np.abs(dl).T @ np.abs(pooled)), dl.sum(axis=0), gamma(B) * np.abs(dl).sum(axis=0)


def head_dgrad_ref(dl, w, HW: int, bf16: bool):
    """dl [B][n_cls], w [n_cls][C] -> (dX [B][HW][C] (bf16: rounded once to bf16), gate)."""
    dl, w = f64(dl), f64(w)
    n_cls = dl.shape[1]
    row = dl @ w / HW
    gate = gamma(n_cls + 1) * (np.abs(dl) @ np.abs(w) / HW)
    if bf16:
        row = round_to(row, "bf16")
        gate = gate + quantum(row, "bf16")
    rep = lambda a: np.repeat(a[:, None, :], HW, axis=1)  # noqa: E731
    return rep(row), rep(gate)


def head_f32(x, w, bias, dl, bf16: bool):
    """The four kernels restated in NumPy float32 in the kernels' own summation order (the CPU check that the gates admit a correct float32
    evaluation).  Returns pooled, logits, dW, db, dX (bf16: float32 values of the bf16 results)."""
    F = np.float32
    x, w, bias, dl = (np.asarray(a, F) for a in (x, w, bias, dl))
    B, HW, C = x.shape
    n_cls = w.shape[0]
    s = np.zeros((B, C), F)
    for q in range(HW):
        s = s + x[:, q, :]
    pooled = s / F(HW)
    acc = np.zeros((B, n_cls, 64), F)
    for c0 in range(0, C, 64):
        lanes = min(64, C - c0)
        acc[:, :, :lanes] = (pooled[:, None, c0:c0 + lanes].astype(np.float64) * w[None, :, c0:c0 + lanes] + acc[:, :, :lanes]).astype(F)   # fma
    m = 32
    while m >= 1:
        acc = acc + acc[:, :, np.arange(64) ^ m]
        m >>= 1
    logits = acc[:, :, 0] + bias[None, :]
    dW, db = np.zeros((n_cls, C), F), np.zeros(n_cls, F)
    for b in range(B):
        dW = (dl[b][:, None].astype(np.float64) * pooled[b][None, :] + dW).astype(F)
        db = db + dl[b]
    t = np.zeros((B, C), F)
    for k in range(n_cls):
        t = (dl[:, k][:, None].astype(np.float64) * w[k][None, :] + t).astype(F)
    t = t / F(HW)
    if bf16:
        t = bf16_bits_to_f32(pack_bf16_ref(t.view(np.uint32)))
    dX = np.repeat(t[:, None, :], HW, axis=1)
    return pooled, logits, dW, db, dX


# (B, HW, C, n_cls) from B in {1, 5}, HW in {4, 49}, C in {512, 2048}, n_cls in {2, 5, 7}: B n_cls = 2, 25, 7, 35, 5, 10, 35 -- none a
# multiple of 4, so the four-logits-per-block grid of fc_fwd_kernel always ends in a partial block; and two B = 64 cases (320 logits)
HEAD_SHAPES = [(1, 4, 512, 2), (5, 4, 512, 5), (1, 49, 512, 7), (5, 49, 512, 7), (1, 4, 2048, 5), (5, 49, 2048, 2), (5, 4, 2048, 7),
               (64, 49, 512, 5), (64, 4, 2048, 5)]


def head_case(B, HW, C, n_cls, bf16):
    rng = np.random.default_rng(B * 1000 + HW * 10 + C + n_cls + bf16)
    x = (np.maximum(rng.standard_normal((B, HW, C)), 0) * 1.5).astype(np.float32)      # a post-ReLU map
    if bf16:
        x = bf16_bits_to_f32(pack_bf16_ref(x.view(np.uint32)))
    w = (rng.standard_normal((n_cls, C)) / np.sqrt(C)).astype(np.float32)
    bias = (rng.standard_normal(n_cls) * 0.1).astype(np.float32)
    dl = (rng.standard_normal((B, n_cls)) / B).astype(np.float32)
    return x, w, bias, dl


def head_check(x, w, bias, dl, bf16, got):
    """[(name, worst |got - want| / gate)] of the five outputs; `got` = (pooled, logits, dW, db, dX) as float32 values."""
    HW = x.shape[1]
    pooled = got[0]
    dw_want, dw_gate, db_want, db_gate = fc_wgrad_ref(dl, pooled)
    pairs = [("pooled", got[0], *pooled_ref(x)), ("logits", got[1], *logits_ref(pooled, w, bias)), ("dW", got[2], dw_want, dw_gate),
             ("db", got[3], db_want, db_gate), ("dX", got[4], *head_dgrad_ref(dl, w, HW, bf16))]
    out = []
    for name, g, want, gate in pairs:
        g = np.asarray(g, np.float64)
        assert g.shape == want.shape, (name, g.shape, want.shape)
        assert np.isfinite(g).all(), name
        out.append((name, float((np.abs(g - want) / np.maximum(gate, 1e-300)).max())))
    return out


CE_SHAPES = [(B, n) for B in (1, 37, 256, 257, 1024) for n in (2, 5)]


# ---- cross-entropy loss ----------------------------------------------------------------------------------------------------------------

def ce_loss_ref(logits, labels):
    """CrossEntropyLoss(mean) and dl = (softmax - onehot) / B in float64 with their gates.  The kernel (ce_loss_kernel), per row:

        m = max l;  s = sum_k expf(l_k - m);  lse = m + logf(s);  term = lse - l_y;  dl_k = (expf(l_k - lse) - [k = y]) / B

    x_k = l_k - m is rounded (u |x_k|, which expf turns into a relative error), expf has EPS_EXPF, the sum of n_cls non-negative terms
    n_cls - 1 additions:        rel(s)  <= sum_k e_k (u |x_k| + EPS_EXPF) / s + gamma(n_cls - 1)          [+ n_cls 2^-149: terms that underflow]
    log turns that into an absolute error, logf adds EPS_LOGF |log s|, the two additions round:
                                E_lse   = rel(s) + EPS_LOGF |log s| + u |lse|,      E_term = E_lse + u |term|
    The loss: each of 256 threads adds its ceil(B / 256) rows, an 8-level tree adds the threads, one division by B:
                                gate    = gamma(ceil(B / 256) + 9) mean |term| + (1 + gamma(...)) mean E_term
    dl: the exponent l_k - lse carries E_lse + u |l_k - lse| into expf as a relative error of p_k = softmax_k, + EPS_EXPF; the subtraction
    of the one-hot and the division by B round:
                                gate_dl = (p_k (E_lse + u |l_k - lse| + EPS_EXPF) (1 + 1e-6) + gamma(2) |p_k - [k = y]|) / B + 2^-149.
    Returns loss, gate, dl, gate_dl."""
    l = f64(logits)
    y = np.asarray(labels, np.int64)
    B, n_cls = l.shape
    m = l.max(axis=1, keepdims=True)
    x = l - m
    e = np.exp(x)
    s = e.sum(axis=1, keepdims=True)
    lse = m + np.log(s)
    ly = np.take_along_axis(l, y[:, None], axis=1)
    term = lse - ly
    rel_s = (e * (U * np.abs(x) + EPS_EXPF)).sum(axis=1, keepdims=True) / s + gamma(max(n_cls - 1, 1)) + n_cls * 2.0 ** -149
    E_lse = rel_s + EPS_LOGF * np.abs(np.log(s)) + U * np.abs(lse)
    E_term = E_lse + U * np.abs(term)
    K = -(-B // 256) + 9
    loss = term.mean()
    gate = gamma(K) * np.abs(term).mean() + (1 + gamma(K)) * E_term.mean()
    p = np.exp(l - lse)
    onehot = np.zeros_like(l)
    onehot[np.arange(B), y] = 1.0
    dl = (p - onehot) / B
    gate_dl = (p * (E_lse + U * np.abs(l - lse) + EPS_EXPF) * (1 + 1e-6) + gamma(2) * np.abs(p - onehot)) / B + 2.0 ** -149
    return float(loss), float(gate), dl, gate_dl


def ce_loss_f32(logits, labels):
    """ce_loss_kernel restated in NumPy float32, in its order: 256 strided partial sums, the LDS tree, the division."""
    F = np.float32
    l = np.asarray(logits, F)
    y = np.asarray(labels, np.int64)
    B, n_cls = l.shape
    m = l.max(axis=1, keepdims=True)
    s = np.zeros((B, 1), F)
    for k in range(n_cls):
        s = s + np.exp(l[:, k:k + 1] - m)
    lse = m + np.log(s)
    term = (lse - np.take_along_axis(l, y[:, None], axis=1))[:, 0]
    red = np.zeros(256, F)
    for b in range(B):
        red[b % 256] = red[b % 256] + term[b]
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    onehot = np.zeros_like(l)
    onehot[np.arange(B), y] = 1
    return red[0] / F(B), (np.exp(l - lse) - onehot) / F(B)


def ce_case(B: int, n_cls: int, seed: int = 0):
    """Logits and labels of a loss case: |logit| ~ 3 at random, and (cycling through the rows 0 .. 4 as far as B reaches; B = 1 takes row
    `seed % 5`) a row of all +80, a row of all -80, a row alternating +80 / -80 (expf of the raw logits overflows: only the max subtraction
    keeps it finite), a row whose logits are all equal, and a row whose true class lies 80 below the maximum."""
    rng = np.random.default_rng(100 * B + n_cls + seed)
    l = (rng.standard_normal((B, n_cls)) * 3).astype(np.float32)
    y = rng.integers(0, n_cls, B)
    special = [np.full(n_cls, 80.0), np.full(n_cls, -80.0), np.where(np.arange(n_cls) % 2 == 0, 80.0, -80.0), np.full(n_cls, 0.625),
               np.concatenate([[-77.5], np.full(n_cls - 1, 2.5)])]
    for i, row in enumerate(special):
        r = 0 if B == 1 else i
        if r < B and (B > 1 or i == seed % 5):
            l[r] = row.astype(np.float32)
            if i == 4:
                y[r] = 0
            if i == 2:
                y[r] = 1      # the true class is the one at -80: the row's loss is 160
    return l, y.astype(np.int64)


# ---- bf16 wire format ---------------------------------------------------------------------------------------------------------------------

LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def wire_inputs() -> np.ndarray:
    """float32 bit patterns: every upper half x the lower halves that decide a rounding (exact, just above, just below a tie, the tie,
    just above it, all ones): 393 216 values, every exponent, both signs, subnormals, infinities and NaNs of every kind."""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    return (hi | np.asarray(LOW_HALVES, np.uint32)[None, :]).reshape(-1)


def pack_bf16_ref(bits: np.ndarray) -> np.ndarray:
    """float32 bits -> bf16 bits by integer round-to-nearest, ties to even: add 0x7FFF + the lowest kept bit, drop 16 bits.  The carry runs
    into the exponent, so a finite value past the largest bf16 becomes infinity and infinities stay.  A NaN stays a NaN (quiet bit set; its
    payload is not part of the contract)."""
    u = np.asarray(bits, np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32)


def unpack_bf16_ref(b: np.ndarray, scale: float) -> np.ndarray:
    """bf16 bits -> float32 value * float32(scale): one IEEE float32 product (subnormal results are kept)."""
    with np.errstate(all="ignore"):
        return bf16_bits_to_f32(b) * np.float32(scale)
