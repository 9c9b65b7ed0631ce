"""Element-wise float64 parity of the bf16 training engine's batch-norm and pooling kernels (train2_kernels.inc, bn_fold.inc) through the
engine's own launch code (t2_bn_fwd / t2_bn_bwd / t2_bn_pool_bwd behind dh_debug_bn2_paths_bf16, dh_debug_bn2_pool_bf16 and
dh_debug_maxpool2_idx_bf16).  Cases, operands and the judge are oracle/bn_cases.py, the reference and the derivation of every gate
oracle/bn_ref.py; tests/test_bn_reference_host.py shows on the CPU that a float32 emulation passes them and planted errors do not.

Per case: every output is prefilled (bf16 0x7FC0, float32 NaN, idx / bits 0xFF) and no prefill may survive; two runs give equal bits; a
map that folds (rows <= 16 384) also runs with fold = 0 and must equal fold = 1 bit for bit in every output; y, dz (pooled, dx) pass
|got - want| <= ulp(want) + gamma_K A element by element with an identical fraction of at least 0.999; bits is the pattern of the stored
y and g_out is dy masked by it, exactly; decided pool windows match in value AND first-maximum position; mean / invstd / dgamma / dbeta
keep the gates of tests/test_gpu_train_kernels.py plus the per-channel any-order summation bound; both caps on undecided elements hold.

Measured on an MI355X (pytest -s; figures of the first run of each case):
25 cases, 4.9 s wall time for the file (26 tests).  identical = share of ALL referenced elements equal to the reference bit for bit (exempt,
by name: every output of the one- and two-row maps and the forward output of the constant channel, oracle/bn_ref.py); worst = largest
|got - want| / gate; the figures agree with the float32 emulation of the host test (invstd to every printed digit).
  case                     y identical  y worst   dz identical  dz worst  invstd rel   dgamma rel  undecided
  r1_c512                  (exempt)     0.853     (exempt)      0.086     5.4e-08      0           0
  r2_c512_res_premasked    (exempt)     0.345     (exempt)      0.356     7.5e-08      4.2e-08     -
  r65_c64                  1            0         1             0         9.7e-08      1.2e-07     0
  r245_c2048_res_gout      0.99994      0.99976   0.99987       0.9998    3.9e-07      1.4e-07     -
  r591_c1024_norelu        0.9998       0.99996   0.99972       0.99975   2.9e-07      1.3e-07     -
  r3139_c64                1            0         0.99982       0.99988   1.3e-07      1.6e-07     0
  r16384_c128_res_gout     0.99995      0.99993   0.99984       0.99988   2.6e-07      9.3e-08     -
  r16385_c128              1            0         0.99993       0.99994   1.6e-07      1.1e-07     0
  r16388_c512_res_gout     0.99995      0.99949   0.99992       0.99936   1.1e-07      1.3e-07     -
  r16385_c2048_norelu      0.99981      0.99994   0.99975       0.99974   7.1e-08      1.2e-07     -
  join_r392_c256           0.99988      0.99219   0.9999        0.99986   1.7e-07      1.3e-07     -
  join_r98_c2048           0.99991      0.99971   0.99988       0.99916   4.3e-07      1.4e-07     -
  join_r16385_c256         0.99994      0.99988   0.99994       0.99989   1.8e-07      1.4e-07     -
  stem tail (pooled / dz)  b1_h2: 1 / 1, 0 undecided windows; b2_h5: 1 / 1, 0.0026; b2_h16: 1 / 1, 0.0066; b1_h17: 1 / 0.99989, 0.0019;
                           b3_h56: 1 / 0.99993 (dz worst 0.9999), 0.0035; b4_h30: 1 / 0.99982 (dz worst 0.984), 0.0056; invstd <= 2.7e-07
  stand-alone max-pool     y and idx exact, dx identical 1 in all six cases
No element of any case is outside its gate, no ReLU pattern is undecided, fold 0 = fold 1 and run 1 = run 2 bit for bit everywhere.
"y identical 1, worst 0" of r65 / r3139 / r16385_c128 (ReLU, no identity, C = 64 / 128) means every element matched: z is bf16-exact, so a
channel holds only a few thousand distinct values of z and none of them lands near a rounding midpoint.  The gate and the planted errors
bite there as anywhere, but the identical fraction has little statistical power on these cases; the wide ones and the ones with an
identity carry it.

FOUND AND FIXED.  With the kernels as they were, r16384_c128_res_gout missed one gate: invstd of channel 83 (mean = 7.9 standard
deviations) was 3.72e-06 off, gate 1e-6.  At the last folded size a row group of bn2_cs_reduce_kernel holds 512 rows; its 32 row lanes
(16 rows each, exact) were added in float32, 31 roundings that left sum z^2 1.2e-07 off, and the one-pass variance E z^2 - mean^2
multiplies that by 1 + (mean / std)^2 = 64.  The lanes of the STATISTICS are now added in double and rounded once (the host test keeps the
comparison); the backward sums, which have no such amplification, keep their float32 order.  Measured after the change: 2.6e-07 (the row above).
"""
import numpy as np
import pytest
import torch

from oracle import bn_cases as bc

pytestmark = pytest.mark.gpu

PREFILL = bc.PREFILL_BF16


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _bf_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).bfloat16().to(dev).contiguous()


def _f_dev(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits16(shape, dev):
    return torch.full(shape, PREFILL, dtype=torch.int16, device=dev)


def _nan32(C, dev):
    return torch.full((C,), float("nan"), dtype=torch.float32, device=dev)


def _np(t):
    if t is None:
        return None
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _run_bn(c, d, dev, fold):
    from deephisto_amd._lib import check, lib
    rows, C = c.rows, c.C
    o = dict(y=_bits16((rows, C), dev), dz=_bits16((rows, C), dev), g_out=_bits16((rows, C), dev) if c.mode == 1 else None,
             bits=torch.full((rows, C // 8), 0xFF, dtype=torch.uint8, device=dev),
             mean=_nan32(C, dev), invstd=_nan32(C, dev), dgamma=_nan32(C, dev), dbeta=_nan32(C, dev),
             mean2=_nan32(C, dev) if c.join else None, invstd2=_nan32(C, dev) if c.join else None)
    check(lib().dh_debug_bn2_paths_bf16(_ptr(d["z"]), _ptr(d["res"]), _ptr(d["gamma"]), _ptr(d["beta"]), c.relu, fold, _ptr(o["y"]),
                                        _ptr(o["bits"]), _ptr(o["mean"]), _ptr(o["invstd"]), _ptr(d["z2"]), _ptr(d["gamma2"]),
                                        _ptr(d["beta2"]), _ptr(o["mean2"]), _ptr(o["invstd2"]), _ptr(d["dy"]), c.mode if c.relu else 0,
                                        _ptr(o["dz"]), _ptr(o["g_out"]), _ptr(o["dgamma"]), _ptr(o["dbeta"]), rows, C, None), "bn2 paths")
    return o


def _same(a, b):
    """Equal bits (NaN-prefilled float32 outputs compare as integers)."""
    return all((a[k] is None and b[k] is None) or torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k],
                                                              b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]) for k in a)


def _differ(a, b):
    return [k for k in a if a[k] is not None and not _same({k: a[k]}, {k: b[k]})]


def _assert_report(rep):
    print("\n" + rep.line())
    assert not rep.failures, "\n".join(rep.failures)


@pytest.mark.parametrize("name", [c.name for c in bc.BN_CASES])
def test_bn_case_matches_float64_reference(dev, name):
    c = bc.BN_BY_NAME[name]
    o = bc.bn_operands(name)
    d = dict(z=_bf_dev(o.z, dev), res=_bf_dev(o.res, dev), dy=_bf_dev(o.dy, dev), z2=_bf_dev(o.z2, dev), gamma=_f_dev(o.gamma, dev),
             beta=_f_dev(o.beta, dev), gamma2=_f_dev(o.gamma2, dev), beta2=_f_dev(o.beta2, dev))
    first, second = _run_bn(c, d, dev, 1), _run_bn(c, d, dev, 1)
    assert _same(first, second), f"{name}: two runs differ in {_differ(first, second)}"
    if c.folds:
        plain = _run_bn(c, d, dev, 0)
        assert _same(first, plain), f"{name}: fold = 0 differs from fold = 1 in {_differ(first, plain)}"
    _assert_report(bc.judge_bn(c, o, {k: _np(v) for k, v in first.items()}))


def _run_pool(c, d, dev):
    from deephisto_amd._lib import check, lib
    B, H, C, Hp = c.B, c.H, c.C, c.Hp
    o = dict(pooled=_bits16((B, Hp, Hp, C), dev), idx=torch.full((B, Hp, Hp, C), 0xFF, dtype=torch.uint8, device=dev),
             dz=_bits16((B, H, H, C), dev), mean=_nan32(C, dev), invstd=_nan32(C, dev), dgamma=_nan32(C, dev), dbeta=_nan32(C, dev))
    check(lib().dh_debug_bn2_pool_bf16(_ptr(d["z"]), _ptr(d["gamma"]), _ptr(d["beta"]), _ptr(o["pooled"]), _ptr(o["idx"]), _ptr(o["mean"]),
                                       _ptr(o["invstd"]), _ptr(d["dpool"]), _ptr(o["dz"]), _ptr(o["dgamma"]), _ptr(o["dbeta"]), B, H, H, C, None),
          "bn2 pool")
    return o


@pytest.mark.parametrize("name", [c.name for c in bc.POOL_CASES])
def test_stem_tail_matches_float64_reference(dev, name):
    c = bc.POOL_BY_NAME[name]
    o = bc.pool_operands(name)
    d = dict(z=_bf_dev(o.z, dev), dpool=_bf_dev(o.dpool, dev), gamma=_f_dev(o.gamma, dev), beta=_f_dev(o.beta, dev))
    first, second = _run_pool(c, d, dev), _run_pool(c, d, dev)
    assert _same(first, second), f"{name}: two runs differ in {_differ(first, second)}"
    _assert_report(bc.judge_pool(c, o, {k: _np(v) for k, v in first.items()}))


def _run_maxpool(c, d, dev):
    from deephisto_amd._lib import check, lib
    B, H, C, Hp = c.B, c.H, c.C, c.Hp
    o = dict(y=_bits16((B, Hp, Hp, C), dev), idx=torch.full((B, Hp, Hp, C), 0xFF, dtype=torch.uint8, device=dev), dx=_bits16((B, H, H, C), dev))
    check(lib().dh_debug_maxpool2_idx_bf16(_ptr(d["x"]), _ptr(o["y"]), _ptr(o["idx"]), _ptr(d["dpool"]), _ptr(o["dx"]), B, H, H, C, None),
          "maxpool2 idx")
    return o


@pytest.mark.parametrize("name", [c.name for c in bc.POOL_CASES])
def test_maxpool_matches_reference(dev, name):
    c = bc.POOL_BY_NAME[name]
    o = bc.pool_operands(name)
    d = dict(x=_bf_dev(o.x, dev), dpool=_bf_dev(o.dpool, dev))
    first, second = _run_maxpool(c, d, dev), _run_maxpool(c, d, dev)
    assert _same(first, second), f"{name}: two runs differ in {_differ(first, second)}"
    _assert_report(bc.judge_maxpool(c, o, {k: _np(v) for k, v in first.items()}))


def test_hooks_name_the_argument_they_refuse(dev):
    from deephisto_amd._lib import lib
    L = lib()
    z = torch.zeros(64, 64, dtype=torch.bfloat16, device=dev)
    f = torch.ones(64, device=dev)
    y, u8 = torch.zeros_like(z), torch.zeros(64, 64, dtype=torch.uint8, device=dev)

    def bn(**kw):
        a = dict(z=z, res=None, gamma=f, beta=f, relu=1, fold=1, y=y, bits=None, mean=f.clone(), invstd=f.clone(), z2=None, gamma2=None,
                 beta2=None, mean2=None, invstd2=None, dy=None, mode=0, dz=None, g_out=None, dgamma=None, dbeta=None, rows=64, C=64)
        a.update(kw)
        p = [_ptr(v) if isinstance(v, torch.Tensor) or v is None else v for v in a.values()]
        return L.dh_debug_bn2_paths_bf16(*p, None), L.dh_last_error().decode()

    assert bn()[0] == 0
    for kw, word in [(dict(fold=2), "fold=2"), (dict(C=72), "C=72"), (dict(rows=0), "rows=0"), (dict(z2=z), "z2_dev"), (dict(relu=3), "relu=3"),
                     (dict(dy=z), "dz_dev"), (dict(g_out=y), "g_out_dev"), (dict(y=None), "y_dev"),
                     (dict(dy=z, dz=y, dgamma=f.clone(), dbeta=f.clone(), mode=5), "relu_mode=5")]:
        rc, msg = bn(**kw)
        assert rc != 0 and word in msg, (kw.keys(), msg)
    rc = L.dh_debug_maxpool2_idx_bf16(_ptr(z), _ptr(y), None, None, None, 1, 8, 8, 64, None)
    assert rc != 0 and "idx_dev" in L.dh_last_error().decode()
    rc = L.dh_debug_maxpool2_idx_bf16(_ptr(z), _ptr(y), _ptr(u8), None, None, 1, 8, 8, 60, None)
    assert rc != 0 and "C=60" in L.dh_last_error().decode()
