"""The batch-norm and pooling cases of the bf16 training engine (tests/test_gpu_bn_bf16_parity.py) with their seeded operands, the judge
that holds a set of outputs to oracle/bn_ref.py, and a float32 emulation of the kernels' arithmetic -- shared with
tests/test_bn_reference_host.py, which shows on the CPU that a plain float32 evaluation passes every gate and that planted errors do not.

Operands.  z is bf16-exact, channel c has standard deviation in [0.5, 1.5] and a mean of 0, 1, 4, 8 standard deviations (c mod 4): the
cancellation between z sc and mean sc, and the one-pass variance, are exercised at every size.  Channel CONST is constant (variance 0,
invstd = 1 / sqrt(eps)) with a bf16-exact beta, so its y must be exactly that beta.  dy = 1e-3 (noise + m_c + r_c xhat), |m_c|, r_c in
[0.5, 2], rounded to bf16: dbeta / n and dgamma xhat / n are then as large as the gradient itself and a wrong k1 or k2 moves every
element.  Pool cases: odd channels are quantised to multiples of 0.25 (exact positive ties), channels with (c / 2) odd have beta = -1.5
(whole windows are zero after the ReLU: ties at zero).
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from oracle import bn_ref as br
from oracle.layer_ref import round_to

CONST = 5                    # the constant channel of every case
CONST_Z, CONST_BETA = 1.5, 0.375
IDENTICAL = 0.999            # IDENTICAL["bf16"] of tests/test_gpu_layer_parity.py
PREFILL_BF16 = 0x7FC0
SELECT_FROM = 8 << 20        # elements from which the elementwise reference covers a selection of rows


class BnCase(NamedTuple):
    name: str
    rows: int
    C: int
    relu: int
    res: bool
    mode: int            # backward ReLU pattern: 0 none / dy pre-masked, 1 from the stored y (+ g_out), 2 recomputed from z
    join: bool = False

    @property
    def folds(self) -> bool:
        return self.rows <= 16384


class PoolCase(NamedTuple):
    name: str
    B: int
    H: int
    C: int
    draw: int = 0        # which seeded draw of the operands (see POOL_CASES)

    @property
    def Hp(self) -> int:
        return (self.H - 1) // 2 + 1


# Forward forms of the engine: ReLU without identity (a block's inner BNs; backward mode 2), ReLU with identity (a block's top BN; mode 1
# with g_out, or mode 0 when the dgrad GEMM masked dy already), no ReLU (downsample BN; mode 0), the join (mode 1).  Each appears on the
# folded path (rows <= 16 384) and on the large-map path.
BN_CASES = [
    BnCase("r1_c512", 1, 512, 1, False, 2),                  # layer 4 at P = 32, one row: n / (n - 1), variance 0 everywhere
    BnCase("r2_c512_res_premasked", 2, 512, 1, True, 0),
    BnCase("r65_c64", 65, 64, 1, False, 2),                  # two row groups, the second with one row
    BnCase("r245_c2048_res_gout", 245, 2048, 1, True, 1),    # ResNet-50 layer 4: 32 slices
    BnCase("r591_c1024_norelu", 591, 1024, 0, False, 0),     # downsample BN
    BnCase("r3139_c64", 3139, 64, 1, False, 2),              # row-group tail not a multiple of 128
    BnCase("r16384_c128_res_gout", 16384, 128, 1, True, 1),  # the last folded size
    BnCase("r16385_c128", 16385, 128, 1, False, 2),          # the first size through bn2_stats / bn2_bwd_reduce and the finalize launches
    BnCase("r16388_c512_res_gout", 16388, 512, 1, True, 1),  # large map, rpi = 4
    BnCase("r16385_c2048_norelu", 16385, 2048, 0, False, 0),  # large map, tpr = 256, rpi = 1; bn2_apply_kernel's grid-stride loop wraps
    BnCase("join_r392_c256", 392, 256, 1, False, 1, True),
    BnCase("join_r98_c2048", 98, 2048, 1, False, 1, True),
    BnCase("join_r16385_c256", 16385, 256, 1, False, 1, True),
]
# b1_h2_c64 is one window of four pixels per channel: a single window with an unsafe element is 1.6 % of its 64 windows, over the 1 % cap,
# and four samples of a channel quantised to 0.25 make 1 + xhat_i xhat_j = 0 exactly in one channel in three, a dz element that is nothing
# but rounding noise.  Its operands are the first seeded draw whose FLOAT64 REFERENCE has neither (`pool_reference_census`; draw 0 has
# five such elements, draws 1 .. 7 one or the other): a property of the inputs, judged without any output of a kernel or of the emulation.
POOL_CASES = [PoolCase("b1_h2_c64", 1, 2, 64, 8), PoolCase("b2_h5_c64", 2, 5, 64), PoolCase("b2_h16_c64", 2, 16, 64),
              PoolCase("b1_h17_c64", 1, 17, 64), PoolCase("b3_h56_c64", 3, 56, 64), PoolCase("b4_h30_c128", 4, 30, 128)]
BN_BY_NAME = {c.name: c for c in BN_CASES}
POOL_BY_NAME = {c.name: c for c in POOL_CASES}

_bf = lambda t: t.bfloat16().float()  # noqa: E731


def bits_to_f64(b) -> np.ndarray:
    return (np.asarray(b, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def f32_to_bits(v) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even (NaN stays NaN)."""
    t = torch.from_numpy(np.ascontiguousarray(v, np.float32)).bfloat16()
    return t.view(torch.int16).numpy().view(np.uint16)


def _params(C: int, g: torch.Generator):
    gam = 0.5 + torch.rand(C, generator=g)
    bet = 0.3 * torch.randn(C, generator=g)
    bet[CONST] = CONST_BETA
    return gam, bet


def _structured(rows: int, C: int, g: torch.Generator) -> torch.Tensor:
    std = 0.5 + torch.rand(C, generator=g)
    m = torch.tensor([0.0, 1.0, 4.0, 8.0])[torch.arange(C) % 4] * std
    z = _bf(torch.randn(rows, C, generator=g) * std + m)
    z[:, CONST] = CONST_Z
    return z


def _gradient(xhat: torch.Tensor, g: torch.Generator) -> torch.Tensor:
    C = xhat.shape[-1]
    sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    mc = sign * (0.5 + 1.5 * torch.rand(C, generator=g))
    rc = 0.5 + 1.5 * torch.rand(C, generator=g)
    return _bf(1e-3 * (torch.randn(xhat.shape, generator=g) + mc + rc * xhat))


def _xhat(z2d: torch.Tensor):
    mu, var = br.column_stats(z2d.numpy())
    return ((z2d - torch.from_numpy(mu).float()) * torch.from_numpy(1.0 / np.sqrt(var + br.EPS)).float()), mu, var


class BnOperands(NamedTuple):
    z: np.ndarray                 # float32 [rows][C], bf16-exact
    res: np.ndarray | None
    gamma: np.ndarray             # float32 [C]
    beta: np.ndarray
    dy: np.ndarray                # float32 [rows][C], bf16-exact; mode 0 with ReLU: already masked by the float64 pattern
    z2: np.ndarray | None         # the join's branch
    gamma2: np.ndarray | None
    beta2: np.ndarray | None
    mu: np.ndarray                # float64 statistics of z (and z2)
    var: np.ndarray
    mu2: np.ndarray | None
    var2: np.ndarray | None


@functools.lru_cache(maxsize=1)
def bn_operands(name: str) -> BnOperands:
    c = BN_BY_NAME[name]
    g = torch.Generator().manual_seed(2000 + BN_CASES.index(c))
    z = _structured(c.rows, c.C, g)
    gam, bet = _params(c.C, g)
    res = _bf(torch.randn(c.rows, c.C, generator=g)) if c.res else None
    xhat, mu, var = _xhat(z)
    dy = _gradient(xhat, g)
    if c.relu and c.mode == 0:      # the engine hands such a BN a gradient its producer masked already
        pre, _ = br.forward(z.numpy(), gam.numpy(), bet.numpy(), mu, 1.0 / np.sqrt(var + br.EPS), None if res is None else res.numpy())
        dy = dy * torch.from_numpy(pre > 0).float()
    z2 = g2 = b2 = mu2 = var2 = None
    if c.join:
        z2 = _structured(c.rows, c.C, g)
        g2, b2 = _params(c.C, g)
        mu2, var2 = br.column_stats(z2.numpy())
        z2, g2, b2 = z2.numpy(), g2.numpy(), b2.numpy()
    return BnOperands(z.numpy(), None if res is None else res.numpy(), gam.numpy(), bet.numpy(), dy.numpy(), z2, g2, b2, mu, var, mu2, var2)


class PoolOperands(NamedTuple):
    z: np.ndarray                 # float32 [B][H][H][C], bf16-exact
    gamma: np.ndarray
    beta: np.ndarray
    dpool: np.ndarray             # float32 [B][Hp][Hp][C], bf16-exact
    mu: np.ndarray
    var: np.ndarray
    x: np.ndarray                 # the stand-alone max-pool's input: rn_bf16(relu(bn(z))) with the float64 statistics, float32


@functools.lru_cache(maxsize=1)
def pool_operands(name: str) -> PoolOperands:
    c = POOL_BY_NAME[name]
    g = torch.Generator().manual_seed(3000 + POOL_CASES.index(c) + 100 * c.draw)
    rows = c.B * c.H * c.H
    z = _structured(rows, c.C, g)
    ch = torch.arange(c.C)
    z = torch.where(ch % 2 == 1, torch.round(z * 4) / 4, z)
    gam, bet = _params(c.C, g)
    bet = torch.where((ch // 2) % 2 == 1, torch.tensor(-1.5), bet)
    xhat, mu, var = _xhat(z)
    xh = xhat.reshape(c.B, c.H, c.H, c.C)[:, 0::2, 0::2]
    assert xh.shape[1] == c.Hp
    dpool = _gradient(xh, g)
    z4 = z.numpy().reshape(c.B, c.H, c.H, c.C)
    pre, _ = br.forward(z4, gam.numpy(), bet.numpy(), mu, 1.0 / np.sqrt(var + br.EPS))
    return PoolOperands(z4, gam.numpy(), bet.numpy(), dpool.numpy(), mu, var, br.stored(pre).astype(np.float32))


def select(rows: int, C: int) -> np.ndarray:
    """Rows held element by element against float64: all, or for the largest maps the first 64, the last 192 and 256 seeded ones (the
    rest is held by the statistics, which use every row, by two-run equality and by the prefill check)."""
    if rows * C < SELECT_FROM:
        return np.arange(rows)
    mid = np.random.default_rng(rows + C).choice(np.arange(64, rows - 192), 256, replace=False)
    return np.unique(np.r_[0:64, mid, rows - 192:rows])


class Report:
    def __init__(self, name: str):
        self.name, self.failures, self.figures = name, [], {}

    def fail(self, msg: str):
        self.failures.append(f"{self.name}: {msg}")

    def line(self) -> str:
        return f"{self.name}: " + ", ".join(f"{k} {v:.5g}" for k, v in self.figures.items())


def _bad_elements(what, got, want, A, ok, rows, layout=("row", "channel")):
    bad = np.argwhere(~ok)
    lines = [f"{what}: {len(bad)} of {ok.size} elements outside the gate; first ({', '.join(layout)}): got / want / A"]
    for ix in bad[:8]:
        t = tuple(ix)
        at = (int(rows[t[0]]),) + tuple(int(v) for v in t[1:])
        lines.append(f"  {at}: {got[t]!r} / {want[t]!r} / {A[t]:.3g}")
    lines.append(f"  {layout[0]}s {np.unique(rows[bad[:, 0]])[:16].tolist()} ({len(np.unique(bad[:, 0]))}), "
                 f"{layout[-1]}s {np.unique(bad[:, -1])[:16].tolist()} ({len(np.unique(bad[:, -1]))})")
    return "\n".join(lines)


def _gate(rep: Report, what: str, got, want, A, K, rows, extra=0.0, stored=None, skip=None, layout=("row", "channel"), exempt=None):
    """The element-wise gate and the identical fraction of one output; `skip`: undecided elements, outside both; `exempt`: elements that are
    pure cancellation by construction (bn_ref, "Identical fraction"), under the gate but outside the fraction."""
    width = br.gate_width(want, A, K, extra)
    ok = np.abs(got - want) <= width          # NaN fails
    keep = np.ones(ok.shape, bool) if skip is None else ~skip
    rep.figures[f"{what} outside"] = float((~(ok | ~keep)).mean())
    if not (ok | ~keep).all():
        rep.fail(_bad_elements(what, got, want, A, ok | ~keep, rows, layout))
    same = (got == (want if stored is None else stored))
    firm = keep if exempt is None else keep & ~np.broadcast_to(exempt, keep.shape)
    rep.figures[f"{what} exempt"] = float((keep & ~firm).mean())
    frac = float(same[firm].mean()) if firm.any() else 1.0
    with np.errstate(invalid="ignore"):
        ratio = np.where(keep, np.abs(got - want) / width, 0.0)
    rep.figures[f"{what} identical"] = frac
    rep.figures[f"{what} worst/gate"] = float(np.nanmax(ratio)) if ratio.size else 0.0
    if frac < IDENTICAL:
        rep.fail(f"{what}: only {frac:.5f} of the elements identical to the reference (floor {IDENTICAL})")


def _exempt(c, forward: bool):
    """Elements outside the identical fraction, by name: every output of a map of one or two rows (variance 0 or xhat = +-1: y is the
    remainder of z sc - mean sc at invstd up to 1 / sqrt(eps), dz is identically 0 in exact arithmetic), and the forward output of the
    constant channel (|z sc| = 1 / sqrt(eps) |gamma z| against a result of |beta + res|).  Everything else counts."""
    col = np.zeros(c.C, bool)
    if getattr(c, "rows", 3) <= 2:
        col[:] = True
    elif forward:
        col[CONST] = True
    return col


def _rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    d = float(np.linalg.norm(a - b))
    return 0.0 if d == 0.0 else d / max(float(np.linalg.norm(b)), 1e-300)


def _stats_gates(rep: Report, tag: str, z2d, mean, invstd, mu, var):
    if not (np.isfinite(mean).all() and np.isfinite(invstd).all()):
        rep.fail(f"{tag}mean / invstd: a prefilled NaN survives")
    e_mean = float(np.abs(np.asarray(mean, np.float64) - mu).max()) / float(np.abs(z2d).max())
    e_is = float(np.abs(np.asarray(invstd, np.float64) * np.sqrt(var + 1e-5) - 1).max())
    rep.figures[f"{tag}mean err/max|z|"] = e_mean
    rep.figures[f"{tag}invstd rel err"] = e_is
    if not e_mean <= 1e-6:
        rep.fail(f"{tag}mean: |got - want| = {e_mean:.3g} max|z| (gate 1e-6)")
    if not e_is <= 1e-6:
        rep.fail(f"{tag}invstd: relative error {e_is:.3g} (gate 1e-6), channel {int(np.abs(np.asarray(invstd, np.float64) * np.sqrt(var + 1e-5) - 1).argmax())}")


def _sum_gates(rep: Report, dgamma, dbeta, sums, rows, mean, invstd, mu, var):
    """dgamma / dbeta: the per-tensor 1e-5 against float64 sums on float64 statistics, and the per-channel any-order bound against the
    sums on the kernel's own statistics."""
    if not (np.isfinite(dgamma).all() and np.isfinite(dbeta).all()):
        rep.fail("dgamma / dbeta: a prefilled NaN survives")
    want64 = (sums["gz"] - mu * sums["g"]) / np.sqrt(var + br.EPS)
    r_g, r_b = _rel(dgamma, want64), _rel(dbeta, sums["g"])
    rep.figures["dgamma rel"] = r_g
    rep.figures["dbeta rel"] = r_b
    if not (r_g <= 1e-5 and r_b <= 1e-5):
        rep.fail(f"dgamma / dbeta: relative L2 {r_g:.3g} / {r_b:.3g} (gate 1e-5)")
    q_g = br.channel_sum_ratio(dgamma, sums["gx"], sums["abs_gx"], sums["loose_gx"], rows)
    q_b = br.channel_sum_ratio(dbeta, sums["g"], sums["abs_g"], sums["loose_g"], rows)
    rep.figures["worst channel sum/bound"] = float(max(q_g.max(), q_b.max()))
    if not (q_g <= 1).all():
        rep.fail(f"dgamma: channels {np.flatnonzero(~(q_g <= 1))[:16].tolist()} outside the summation bound, worst {q_g.max():.3g}")
    if not (q_b <= 1).all():
        rep.fail(f"dbeta: channels {np.flatnonzero(~(q_b <= 1))[:16].tolist()} outside the summation bound, worst {q_b.max():.3g}")


def judge_bn(c: BnCase, o: BnOperands, out: dict) -> Report:
    """out: y, dz, g_out (None unless mode 1), bits -- bf16 bits / bytes as numpy; mean, invstd, dgamma, dbeta (mean2, invstd2) float32."""
    rep = Report(c.name)
    rows, C = c.rows, c.C
    for k in ("y", "dz") + (("g_out",) if out.get("g_out") is not None else ()):
        n = int((out[k] == PREFILL_BF16).sum())
        if n:
            rep.fail(f"{k}: {n} elements never written (rows {np.unique(np.argwhere(out[k] == PREFILL_BF16)[:, 0])[:16].tolist()})")
    mean, invstd = out["mean"], out["invstd"]
    _stats_gates(rep, "", o.z, mean, invstd, o.mu, o.var)
    sel = select(rows, C)
    zs = o.z[sel]
    y_all = bits_to_f64(out["y"])
    got = y_all[sel]
    if c.join:
        _stats_gates(rep, "branch ", o.z2, out["mean2"], out["invstd2"], o.mu2, o.var2)
        want, A, extra, stored = br.join(zs, (o.gamma, o.beta, mean, invstd), o.z2[sel], (o.gamma2, o.beta2, out["mean2"], out["invstd2"]))
        _gate(rep, "y", got, want, A, br.K_FWD, sel, extra, stored, exempt=_exempt(c, True))
    else:
        pre, A = br.forward(zs, o.gamma, o.beta, mean, invstd, None if o.res is None else o.res[sel])
        _gate(rep, "y", got, br.stored(pre, bool(c.relu)), A, br.K_FWD, sel, exempt=_exempt(c, True))
        if o.res is None:
            cb = float(round_to(max(CONST_BETA, 0.0), "bf16"))
            if not (y_all[:, CONST] == cb).all():
                rep.fail(f"y: the constant channel {CONST} is not bf16(beta) = {cb} in rows {np.flatnonzero(y_all[:, CONST] != cb)[:16].tolist()}")
    if out.get("bits") is not None:
        wrong = np.argwhere(out["bits"] != br.pack_bits(out["y"]))
        if len(wrong):
            rep.fail(f"bits: {len(wrong)} bytes differ from the pattern of the stored y; first (row, byte) {wrong[:8].tolist()}")
    # backward
    dy = o.dy
    loose_mag = None
    loose = None
    if c.mode == 1:
        keep = y_all > 0
        g = np.where(keep, dy, np.float32(0))
        if out.get("g_out") is not None:
            dy_bits = f32_to_bits(dy)
            wrong = np.argwhere(out["g_out"] != np.where(keep, dy_bits, np.uint16(0)))
            if len(wrong):
                rep.fail(f"g_out: {len(wrong)} elements differ from dy masked by the stored y; first (row, channel) {wrong[:8].tolist()}")
    elif c.mode == 2:
        pre_all, A_all = br.forward(o.z, o.gamma, o.beta, mean, invstd)
        g = np.where(pre_all > 0, dy, np.float32(0))
        loose = br.undecided(pre_all, A_all)
        loose_mag = np.where(loose, np.abs(dy), np.float32(0))
        share = float(loose.mean())
        rep.figures["undecided share"] = share
        if share > br.UNDECIDED_CAP:
            rep.fail(f"{share:.3g} of the elements have a ReLU pattern float32 cannot decide (cap {br.UNDECIDED_CAP})")
    else:
        g = dy
    sums = br.column_grad_sums(o.z, g, mean, invstd, loose_mag)
    _sum_gates(rep, out["dgamma"], out["dbeta"], sums, rows, mean, invstd, o.mu, o.var)
    dz, A = br.backward(zs, g[sel], o.gamma, mean, invstd, out["dgamma"], out["dbeta"], rows)
    _gate(rep, "dz", bits_to_f64(out["dz"])[sel], round_to(dz, "bf16"), A, br.K_BWD, sel, skip=None if loose is None else loose[sel],
          exempt=_exempt(c, False))
    return rep


def judge_pool(c: PoolCase, o: PoolOperands, out: dict) -> Report:
    """out: pooled, dz (bf16 bits), idx (bytes), mean, invstd, dgamma, dbeta."""
    rep = Report(c.name)
    B, H, C, Hp = c.B, c.H, c.C, c.Hp
    n = B * H * H
    for k in ("pooled", "dz"):
        if int((out[k] == PREFILL_BF16).sum()):
            rep.fail(f"{k}: {int((out[k] == PREFILL_BF16).sum())} elements never written")
    mean, invstd = out["mean"], out["invstd"]
    _stats_gates(rep, "", o.z.reshape(n, C), mean, invstd, o.mu, o.var)
    pre, A = br.forward(o.z, o.gamma, o.beta, mean, invstd)
    want, pos = br.pool(br.stored(pre))
    und = br.pool_any(br.unsafe(pre, A))
    imgs = np.arange(B)
    lay = ("image", "oy", "ox", "channel")
    got, idx = bits_to_f64(out["pooled"]), np.asarray(out["idx"])
    _gate(rep, "pooled", got, want, br.pool_max(A), br.K_FWD, imgs, layout=lay, exempt=_exempt(c, True))
    share = float(und.mean())
    rep.figures["undecided windows"] = share
    if share > br.WINDOW_CAP:
        rep.fail(f"{share:.3g} of the windows hold an element float32 cannot decide (cap {br.WINDOW_CAP})")
    oy, ox = np.arange(Hp)[None, :, None, None], np.arange(Hp)[None, None, :, None]
    iy, ix = 2 * oy + idx.astype(np.int64) // 3 - 1, 2 * ox + idx.astype(np.int64) % 3 - 1
    if not ((idx <= 8) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < H)).all():
        rep.fail(f"idx: {int((~((idx <= 8) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < H))).sum())} positions outside their window or the map")
    wrong = ~und & ((got != want) | (idx != pos))
    if wrong.any():
        w = np.argwhere(wrong)
        rep.fail(f"pool: {len(w)} decided windows differ in value or position; first (image, oy, ox, channel): got value / position, want\n" +
                 "\n".join(f"  {tuple(int(v) for v in t)}: {got[tuple(t)]!r} / {int(idx[tuple(t)])}, {want[tuple(t)]!r} / {int(pos[tuple(t)])}" for t in w[:8]))
    pool_backward_gates(rep, c, o, out, pre, A, pos, und)
    return rep


def pool_backward_gates(rep: Report, c: PoolCase, o: PoolOperands, out: dict, pre, A, pos, und):
    """The backward half of judge_pool (also the stem tail of a whole step, oracle/step_bwd_ref.py): dz, dgamma, dbeta of `out` against the
    pooled gradient o.dpool scattered to the reference's positions `pos`; `und`: the undecided windows."""
    B, H, C, Hp = c.B, c.H, c.C, c.Hp
    n = B * H * H
    imgs = np.arange(B)
    mean, invstd = out["mean"], out["invstd"]
    # backward: the pooled gradient scattered to the REFERENCE's positions, masked by pre > 0
    dY, T = br.pool_scatter(o.dpool, pos, H, H), br.pool_scatter(o.dpool, pos, H, H, absolute=True)
    on = pre > 0
    g, T = np.where(on, dY, 0.0), np.where(on, T, 0.0)
    # a gradient of an undecided window may land on any pixel under it; an undecided ReLU pattern may pass or stop what lands there
    loose = br.window_cover(und, H, H) | (br.undecided(pre, A) & (T > 0))
    reach = np.zeros((B, 2 * Hp + 1, 2 * Hp + 1, C))
    for k in range(9):
        reach[:, k // 3:k // 3 + 2 * Hp:2, k % 3:k % 3 + 2 * Hp:2] += np.abs(o.dpool)
    loose_mag = np.where(loose, reach[:, 1:H + 1, 1:H + 1], 0.0)      # everything that can reach the pixel
    rep.figures["dz elements left out"] = float(loose.mean())
    sums = br.column_grad_sums(o.z.reshape(n, C), g.reshape(n, C), mean, invstd, loose_mag.reshape(n, C))
    _sum_gates(rep, out["dgamma"], out["dbeta"], sums, n, mean, invstd, o.mu, o.var)
    dz, Ab = br.backward(o.z, g, o.gamma, mean, invstd, out["dgamma"], out["dbeta"], n, g_terms=T)
    _gate(rep, "dz", bits_to_f64(out["dz"]), round_to(dz, "bf16"), Ab, br.K_POOL_BWD, imgs, skip=loose, layout=("image", "y", "x", "channel"))
    return rep


def pool_reference_census(c: PoolCase, o: PoolOperands):
    """(elements of the exact dz that float32 cannot determine: gamma_K A >= ulp(dz) / 2; windows holding an unsafe element) of a pool case,
    from the float64 reference on float64 statistics alone."""
    from oracle.layer_ref import gamma, quantum
    n = c.B * c.H * c.H
    inv = 1.0 / np.sqrt(o.var + br.EPS)
    pre, A = br.forward(o.z, o.gamma, o.beta, o.mu, inv)
    _, pos = br.pool(br.stored(pre))
    on = pre > 0
    g = np.where(on, br.pool_scatter(o.dpool, pos, c.H, c.H), 0.0)
    T = np.where(on, br.pool_scatter(o.dpool, pos, c.H, c.H, absolute=True), 0.0)
    s = br.column_grad_sums(o.z.reshape(n, c.C), g.reshape(n, c.C), o.mu, inv)
    dz, Ab = br.backward(o.z, g, o.gamma, o.mu, inv, s["gx"], s["g"], n, g_terms=T)
    noise = (gamma(br.K_POOL_BWD) * Ab >= quantum(round_to(dz, "bf16"), "bf16") / 2) & (Ab > 0)
    return int(noise.sum()), int(br.pool_any(br.unsafe(pre, A)).sum())


def judge_maxpool(c: PoolCase, o: PoolOperands, out: dict) -> Report:
    """The stand-alone max-pool on x = o.x: y and idx exact, dx within ulp + gamma_3 sum|terms|.  out: y, dx (bf16 bits), idx."""
    rep = Report(c.name + " maxpool")
    for k in ("y", "dx"):
        if int((out[k] == PREFILL_BF16).sum()):
            rep.fail(f"{k}: {int((out[k] == PREFILL_BF16).sum())} elements never written")
    want, pos = br.pool(o.x)
    got = bits_to_f64(out["y"])
    if not ((got == want) & (np.asarray(out["idx"]) == pos)).all():
        w = np.argwhere((got != want) | (np.asarray(out["idx"]) != pos))
        rep.fail(f"maxpool: {len(w)} windows differ in value or position; first (image, oy, ox, channel) {w[:8].tolist()}")
    dx = br.pool_scatter(o.dpool, pos, c.H, c.H)
    T = br.pool_scatter(o.dpool, pos, c.H, c.H, absolute=True)
    _gate(rep, "dx", bits_to_f64(out["dx"]), round_to(dx, "bf16"), T, br.K_POOL_DX, np.arange(c.B), layout=("image", "y", "x", "channel"))
    return rep


# ---- a float32 emulation of the kernels' arithmetic (the host test; `plant` names an error to put in) -----------------------------------
f32 = np.float32


def _fma(a, b, c):
    """float32 fma of float32 arrays: the product of a bf16-exact factor is exact in double."""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def _colsum32(x32, small: bool, lanes64: bool = True):
    """Column sums in the engine's order of additions: float32 partial rows, added in double.  small (maps of up to 16 384 rows, the
    channel-sliced reductions): a partial row per row group, in it 32 lanes that each add every 32nd row in turn; the lanes are added in
    index order, in double and rounded once for the statistics (lanes64; bn2_cs_reduce_kernel<0>), in float32 for the backward sums
    (<1>).  With float32 lanes the one-pass variance misses its gate at 16 384 x 128: invstd 3.72e-6 off on a channel whose mean is 8
    standard deviations, where var = E z^2 - mean^2 multiplies the error of sum z^2 by 65 (what the engine returned before its
    statistics' lanes went to double; tests/test_bn_reference_host.py keeps the comparison).  Otherwise (bn2_stats_kernel /
    bn2_bwd_reduce_kernel): nb workgroups of rpi row lanes, lane l of workgroup b adds rows (b + k nb) rpi + l, k = 0, 1, ...; the lanes
    are added in index order.  numpy adds the slices of a leading axis one after another."""
    rows, C = x32.shape
    x32 = np.ascontiguousarray(x32, f32)

    def lanes(blk, shape):
        pad = int(np.prod(shape[1:])) * -(-len(blk) // int(np.prod(shape[1:]))) - len(blk)
        if pad:
            blk = np.concatenate([blk, np.zeros((pad, C), f32)])
        return blk.reshape(-1, *shape[1:], C).sum(0, dtype=f32)

    if small:
        nrg = max(1, min(32, 512 // (C // 64), (rows + 63) // 64))
        rpg = -(-rows // nrg)
        parts = [lanes(x32[i:i + rpg], (0, 32)) for i in range(0, rows, rpg)]
        parts = [p.astype(np.float64).sum(0).astype(f32) if lanes64 else p.sum(0, dtype=f32) for p in parts]
    else:
        tpr = min(C // 8, 256)
        rpi = 256 // tpr
        nb = max(1, min(512, -(-rows // rpi), max(256, rows * C * 2 // (48 * 1024))))
        parts = lanes(x32, (0, nb, rpi)).sum(1, dtype=f32)
    return np.asarray(parts, np.float64).sum(0)


def _emulate_stats(z, gam, bet, small: bool):
    n = z.shape[0]
    s1, s2 = _colsum32(z, small), _colsum32(z * z, small)
    mu = s1 / n
    var = np.maximum(s2 / n - mu * mu, 0.0)
    inv = (1.0 / np.sqrt(var + br.EPS)).astype(f32)
    mean = mu.astype(f32)
    sc = (gam * inv).astype(f32)
    sh = (bet - (mean * sc).astype(f32)).astype(f32)
    return mean, inv, sc, sh


def _emulate_bwd_coef(g, z, gam, mean, inv, n, small: bool):
    xh = ((z - mean).astype(f32) * inv).astype(f32)
    s1, s2 = _colsum32(g, small, False), _colsum32((g * xh).astype(f32), small, False)
    a = gam.astype(np.float64) * inv.astype(np.float64)
    b1 = -a * inv.astype(np.float64) * s2 / n
    return a.astype(f32), b1.astype(f32), (-a * s1 / n - b1 * mean.astype(np.float64)).astype(f32), s2.astype(f32), s1.astype(f32)


def emulate_bn(c: BnCase, o: BnOperands, plant: str | None = None) -> dict:
    mean, inv, sc, sh = _emulate_stats(o.z, o.gamma, o.beta, c.folds)
    out = {"mean": mean, "invstd": inv}
    v = _fma(o.z, sc, sh)
    if c.join:
        mean2, inv2, sc2, sh2 = _emulate_stats(o.z2, o.gamma2, o.beta2, c.folds)
        out.update(mean2=mean2, invstd2=inv2)
        r = _fma(o.z2, sc2, sh2)
        if plant != "join_no_inner_rounding":
            r = bits_to_f64(f32_to_bits(r)).astype(f32)
        v = v + r
    if o.res is not None:
        v = v + o.res
    if c.relu:
        v = np.maximum(v, f32(0))
    if plant == "small_scaled":
        v = np.where(np.abs(v) < 0.05, v * f32(1.2), v)
    y = f32_to_bits(v)
    if plant == "swap_channels":
        y[:, 8:16] = y[:, 15:7:-1].copy()
    if plant == "last_row_unwritten":
        y[-1] = PREFILL_BF16
    if plant == "last_row_stale":
        y[-1] = y[-2]
    out["y"] = y
    out["bits"] = br.pack_bits(y)
    if plant == "bits_swapped":
        b = out["bits"]
        out["bits"] = (b & 0xFC) | ((b & 1) << 1) | ((b >> 1) & 1)
    yv = bits_to_f64(y)
    if c.mode == 1:
        g = np.where(yv > 0, o.dy, f32(0))
        out["g_out"] = f32_to_bits(g)
    elif c.mode == 2:
        g = np.where(_fma(o.z, sc, sh) > 0, o.dy, f32(0))
    else:
        g = o.dy
    k0, k1, k2, out["dgamma"], out["dbeta"] = _emulate_bwd_coef(g, o.z, o.gamma, mean, inv, c.rows, c.folds)
    if plant == "no_projection":
        k1, k2 = k1 * f32(0), k2 * f32(0)
    if plant == "k1_scaled":
        k1 = k1 * f32(1.02)
    if plant == "k2_scaled":
        k2 = k2 * f32(0.98)
    dz = f32_to_bits(_fma(k0, g, _fma(k1, o.z, k2)))
    if plant == "last_row_unwritten":
        dz[-1] = PREFILL_BF16
    if plant == "last_row_stale":
        dz[-1] = dz[-2]
    out["dz"] = dz
    return out


def _pool32(r, second_on_tie: bool = False):
    best, pos = br.pool(r)
    if second_on_tie:     # the planted error: where a window holds its maximum more than once, the SECOND such element in row-major order
        P, Ho, Wo = br._padded(np.asarray(r, np.float64), -np.inf)
        seen = np.zeros(best.shape, np.int64)
        for k in range(9):
            seen += P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] == best
            pos = np.where((seen == 2) & (P[:, k // 3:k // 3 + 2 * Ho:2, k % 3:k % 3 + 2 * Wo:2] == best), np.uint8(k), pos)
            seen = np.where(seen == 2, 3, seen)      # taken: later maxima no longer count as the second
    return best, pos


def emulate_pool(c: PoolCase, o: PoolOperands, plant: str | None = None) -> dict:
    n = c.B * c.H * c.H
    z2 = o.z.reshape(n, c.C)
    mean, inv, sc, sh = _emulate_stats(z2, o.gamma, o.beta, False)
    v = _fma(o.z, sc, sh)
    r = bits_to_f64(f32_to_bits(np.maximum(v, f32(0))))
    best, pos = _pool32(r, plant == "second_on_tie")
    dY = br.pool_scatter(o.dpool, pos, c.H, c.H).astype(f32)      # at most four bf16 terms: the float32 sum is exact or one rounding
    g = np.where(v > 0, dY, f32(0))
    k0, k1, k2, dgamma, dbeta = _emulate_bwd_coef(g.reshape(n, c.C), z2, o.gamma, mean, inv, n, False)
    dz = f32_to_bits(_fma(k0, g, _fma(k1, o.z, k2)))
    return {"mean": mean, "invstd": inv, "pooled": f32_to_bits(best.astype(f32)), "idx": pos, "dz": dz, "dgamma": dgamma, "dbeta": dbeta}


def emulate_maxpool(c: PoolCase, o: PoolOperands, plant: str | None = None) -> dict:
    best, pos = _pool32(o.x, plant == "second_on_tie")
    dx = br.pool_scatter(o.dpool, pos, c.H, c.H).astype(f32)
    return {"y": f32_to_bits(best.astype(f32)), "idx": pos, "dx": f32_to_bits(dx)}
