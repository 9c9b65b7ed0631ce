"""Element-wise float64 parity of the training step's tail that is not a convolution: the classifier head of both engines
(avgpool_kernel / avgpool2_kernel, fc_fwd_kernel, fc_wgrad_kernel, avgpool_fc_dgrad_kernel / avgpool_fc_dgrad2_kernel through the
dh_debug_head hook), dh_ce_loss alone, and the bf16 gradient wire format (dh_grad_pack_bf16 / dh_grad_unpack_bf16).

References and gates: oracle/head_ref.py (K and A of every gate counted from the kernels' expressions, stated there; self-checked on the
CPU by tests/test_head_ref_host.py).  Nothing in a gate comes from what a kernel returns.

  head   pooled, logits, dW, db, dX against float64 on the same operands (bf16 x taken as its exact value; logits and dW from the pooled
         features the kernels read), gamma(K) A with K = HW, C, B, B, n_cls + 1 (the division by HW is a rounding after the n_cls
         multiply-adds), + one bf16 unit on the bf16 dX.  Two runs into NaN-prefilled outputs: equal bits, no prefill left.
  loss   B in {1, 37, 256, 257, 1024} x n_cls in {2, 5}: rows of all +80, all -80, alternating +-80, all equal, a true class 80 below the
         maximum (head_ref.ce_case); loss and dl, with and without the dl pointer.
  wire   pack: all 65 536 upper halves x six lower halves, bit-equal to integer round-to-nearest-even (overflow to infinity, infinities
         kept), every NaN a NaN; unpack: all 65 536 patterns x scale {1, 1/8, 1/3}, bit-equal to the float32 product, subnormals included;
         n = 0, 4 and 4 (256 * 4096 + 3); refusals by argument name; guard bytes beyond n untouched.

Measured on an MI355X, worst |got - want| / gate (file: 2.8 s wall for the 37 tests):
  head   pooled <= 0.54, logits <= 0.001 (K = C counts a serial chain; the kernel's is C / 64 + 7), dW <= 0.995 (B = 1: one rounding
         against gamma(1)), db <= 0.25, float32 dX <= 0.74, bf16 dX 0 except one element exactly one bf16 unit off at (64, 4, 2048, 5): 1.000.
         Bit for bit the values of the NumPy restatement in oracle/head_ref.py.
  loss   <= 0.30 of the gate at every shape, dl <= 0.51; the +-80 rows give 160.0, 80.0 and log(n_cls) exactly or to the last bit.
  wire   pack and unpack bit-equal on every pattern; the device keeps subnormal products (254 / 1022 / 638 of them at scale 1, 1/8, 1/3).
         Before this test the pack kernel turned NaNs 0x7F80_0001 .. 0x7F80_7FFF into infinity and 0x7FFF_8000 .. into a signed zero (the
         carry of the rounding add); dh_grad_pack_bf16 now truncates and quiets NaNs.
"""
import numpy as np
import pytest
import torch

from oracle import head_ref as hr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bf16_dev(x_f32_exact, dev):
    """float32 values that are exact in bf16 -> uint16 bits on the device (as int16 storage)."""
    bits = (np.ascontiguousarray(x_f32_exact).view(np.uint32) >> 16).astype(np.uint16)
    return _t(bits.view(np.int16), dev)


def _run_head(dev, x, w, bias, dl, bf16):
    from deephisto_amd._lib import check, lib
    B, HW, C = x.shape
    n_cls = w.shape[0]
    xd = _bf16_dev(x, dev) if bf16 else _t(x, dev)
    wd, bd, dld = _t(w, dev), _t(bias, dev), _t(dl, dev)
    nan = float("nan")
    pooled = torch.full((B, C), nan, device=dev)
    logits = torch.full((B, n_cls), nan, device=dev)
    dw = torch.full((n_cls, C), nan, device=dev)
    db = torch.full((n_cls,), nan, device=dev)
    dx = torch.full((B, HW, C), -1, dtype=torch.int16, device=dev) if bf16 else torch.full((B, HW, C), nan, device=dev)   # 0xFFFF: a bf16 NaN
    check(lib().dh_debug_head(xd.data_ptr(), int(bf16), wd.data_ptr(), bd.data_ptr(), dld.data_ptr(), pooled.data_ptr(), logits.data_ptr(),
                              dw.data_ptr(), db.data_ptr(), dx.data_ptr(), B, HW, C, n_cls, None), "dh_debug_head")
    dxv = hr.bf16_bits_to_f32(dx.cpu().numpy().view(np.uint16)) if bf16 else dx.cpu().numpy()
    return [pooled.cpu().numpy(), logits.cpu().numpy(), dw.cpu().numpy(), db.cpu().numpy(), dxv]


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("B,HW,C,n_cls", hr.HEAD_SHAPES)
def test_head_kernels(dev, B, HW, C, n_cls, bf16):
    x, w, bias, dl = hr.head_case(B, HW, C, n_cls, bf16)
    runs = [_run_head(dev, x, w, bias, dl, bool(bf16)) for _ in range(2)]
    for a, b in zip(*runs):
        assert not np.isnan(a).any()                                   # no prefill left: every element was written
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))    # two runs, equal bits
    res = hr.head_check(x, w, bias, dl, bool(bf16), runs[0])
    print(f"[head] B={B} HW={HW} C={C} n_cls={n_cls} {'bf16' if bf16 else 'f32'}: |got - want| / gate: " + ", ".join(f"{n} {r:.3f}" for n, r in res))
    assert all(r <= 1.0 for _, r in res), res


def test_head_hook_refuses_bad_arguments_by_name(dev):
    from deephisto_amd._lib import lib
    x, w, bias, dl = hr.head_case(1, 4, 512, 2, 0)
    t = [_t(a, dev) for a in (x, w, bias, dl)]
    out = [torch.zeros(n, device=dev) for n in (512, 2, 1024, 2, 2048)]
    ptr = lambda ts: [a.data_ptr() for a in ts]  # noqa: E731

    def call(x_bf16=0, B=1, HW=4, C=512, n_cls=2, null=None):
        a = [t[0].data_ptr(), x_bf16, *ptr(t[1:]), *ptr(out), B, HW, C, n_cls, None]
        if null is not None:
            a[null] = None
        return lib().dh_debug_head(*a), lib().dh_last_error()

    assert call()[0] == 0
    for kw, word in ((dict(x_bf16=2), b"x_bf16"), (dict(B=0), b"B="), (dict(HW=0), b"HW="), (dict(C=516), b"C="), (dict(C=0), b"C="),
                     (dict(n_cls=0), b"n_cls="), (dict(null=0), b"x_dev"), (dict(null=4), b"dlogits_dev"), (dict(null=9), b"dx_dev")):
        rc, msg = call(**kw)
        assert rc == -22 and word in msg, (kw, rc, msg)


# ---- dh_ce_loss ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("B,n_cls", hr.CE_SHAPES)
def test_ce_loss_every_row(dev, B, n_cls):
    from deephisto_amd.models.patch_cls_simple.engine import ce_loss
    for seed in range(5 if B == 1 else 1):
        l, y = hr.ce_case(B, n_cls, seed)
        want, gate, want_dl, gate_dl = hr.ce_loss_ref(l, y)
        ld, yd = _t(l, dev), _t(y, dev)
        loss, dl = ce_loss(ld, yd, want_grad=True)
        alone = ce_loss(ld, yd)                          # without the dl pointer
        got, got_dl = float(loss.double()), dl.cpu().numpy().astype(np.float64)
        r1, r2 = abs(got - want) / gate, float((np.abs(got_dl - want_dl) / gate_dl).max())
        print(f"[ce] B={B} n_cls={n_cls} seed={seed}: loss {got!r} want {want!r}: |got - want| / gate = {r1:.3f}; dl {r2:.3f}")
        assert np.isfinite(got) and np.isfinite(got_dl).all()
        assert r1 <= 1.0 and r2 <= 1.0
        assert torch.equal(alone, loss)


# ---- bf16 gradient wire format -----------------------------------------------------------------------------------------------------------

GUARD = 64


def _pack(dev, bits_u32, n=None):
    """dh_grad_pack_bf16 of float32 bit patterns into a guarded destination; returns (rc, bf16 bits [n], guard intact)."""
    from deephisto_amd._lib import lib
    n = bits_u32.size if n is None else n
    src = _t(bits_u32.view(np.int32), dev)
    dst = torch.full((n + GUARD,), 0x5A5A, dtype=torch.int16, device=dev)
    rc = lib().dh_grad_pack_bf16(src.data_ptr(), dst.data_ptr(), n, None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint16)
    return rc, out[:n], bool((out[n:] == 0x5A5A).all())


def _unpack(dev, bits_u16, scale, n=None):
    from deephisto_amd._lib import lib
    n = bits_u16.size if n is None else n
    src = _t(bits_u16.view(np.int16), dev)
    dst = torch.full((n + GUARD,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    rc = lib().dh_grad_unpack_bf16(src.data_ptr(), dst.data_ptr(), n, scale, None)
    torch.cuda.synchronize()
    out = dst.cpu().numpy().view(np.uint32)
    return rc, out[:n], bool((out[n:] == 0x5A5A5A5A).all())


def test_grad_pack_bf16_every_upper_half(dev):
    bits = hr.wire_inputs()
    rc, got, guard = _pack(dev, bits)
    assert rc == 0 and guard
    want = hr.pack_bf16_ref(bits)
    nan = np.isnan(bits.view(np.float32))
    diff = np.nonzero(got[~nan] != want[~nan])[0]
    assert diff.size == 0, [(hex(int(bits[~nan][i])), hex(int(got[~nan][i])), hex(int(want[~nan][i]))) for i in diff[:8]]
    lost = nan & ~np.isnan(hr.bf16_bits_to_f32(got))
    assert not lost.any(), [(hex(int(bits[i])), hex(int(got[i]))) for i in np.nonzero(lost)[0][:8]]      # every NaN stays a NaN
    big = np.array([0x7F7F8000, 0xFF7F8000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, 0x7F7F7FFF, 0, 0], np.uint32)
    assert _pack(dev, big)[1].tolist()[:6] == [0x7F80, 0xFF80, 0x7F80, 0x7F80, 0xFF80, 0x7F7F]


@pytest.mark.parametrize("scale", [1.0, 1 / 8, 1 / 3])
def test_grad_unpack_bf16_every_pattern(dev, scale):
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    rc, got, guard = _unpack(dev, b, scale)
    assert rc == 0 and guard
    want = hr.unpack_bf16_ref(b, scale)
    nan = np.isnan(want)
    assert np.isnan(got.view(np.float32)[nan]).all()
    diff = np.nonzero(got[~nan] != want.view(np.uint32)[~nan])[0]
    sub = (np.abs(want) > 0) & (np.abs(want) < 2.0 ** -126)
    print(f"[wire] unpack scale {scale}: {int(sub.sum())} subnormal results, {diff.size} mismatches")
    assert diff.size == 0, [(hex(int(b[~nan][i])), hex(int(got[~nan][i])), hex(int(want.view(np.uint32)[~nan][i]))) for i in diff[:8]]


@pytest.mark.parametrize("n", [0, 4, 4 * (256 * 4096 + 3)])
def test_grad_wire_sizes_and_guards(dev, n):
    """n = 0 launches nothing, n = 4 is one thread, 4 (256 * 4096 + 3) is three granules past one pass of the capped grid."""
    rng = np.random.default_rng(n)
    bits = rng.integers(0, 2 ** 32, max(n, 4), dtype=np.uint64).astype(np.uint32)
    bits[(bits & 0x7F800000) == 0x7F800000] &= 0x3FFFFFFF        # finite values: NaN payloads are not part of the contract
    rc, got, guard = _pack(dev, bits, n)
    assert rc == 0 and guard
    assert np.array_equal(got, hr.pack_bf16_ref(bits[:n]))
    b16 = (bits >> 16).astype(np.uint16)
    rc, back, guard = _unpack(dev, b16, 1 / 3, n)
    assert rc == 0 and guard
    assert np.array_equal(back, hr.unpack_bf16_ref(b16[:n], 1 / 3).view(np.uint32))


def test_grad_wire_refusals_name_the_argument(dev):
    from deephisto_amd._lib import lib
    f = torch.zeros(64, device=dev)
    h = torch.zeros(64, dtype=torch.int16, device=dev)
    L = lib()
    # evaluated one at a time: dh_last_error holds the latest message only
    calls = [(lambda: L.dh_grad_pack_bf16(f.data_ptr(), h.data_ptr(), 6, None), b"n=6"),
             (lambda: L.dh_grad_pack_bf16(f.data_ptr() + 4, h.data_ptr(), 8, None), b"src_dev"),
             (lambda: L.dh_grad_pack_bf16(f.data_ptr(), h.data_ptr() + 2, 8, None), b"dst_dev"),
             (lambda: L.dh_grad_unpack_bf16(h.data_ptr(), f.data_ptr(), 7, 1.0, None), b"n=7"),
             (lambda: L.dh_grad_unpack_bf16(h.data_ptr() + 4, f.data_ptr(), 8, 1.0, None), b"src_dev"),
             (lambda: L.dh_grad_unpack_bf16(h.data_ptr(), f.data_ptr() + 8, 8, 1.0, None), b"dst_dev")]
    for fn, word in calls:
        assert fn() == -22 and word in L.dh_last_error(), word
    torch.cuda.synchronize()
    assert not f.any() and not h.any()
