"""Per-kernel parity of the float32 training engine's backward building blocks (VERDICT r1 #3 iii).

Every kernel that dh_resnet18_backward launches is run alone through its debug hook (include/deephisto_hip.h, "debug")
on random data and held against torch autograd on the CPU in float64: relative L2 error <= 1e-5 per output tensor
(float32 MFMA products are exact, sums of up to ~10^4 terms in float32: ~sqrt(K) * 6e-8).  The whole-network tests
(tests/test_gpu_train.py) can only afford 2e-2 because ReLU patterns flip between two float32 implementations; these
tests cannot hide a 1 % error in a BN coefficient or a wgrad edge tap."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 1e-5


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rel(got, want):
    want = want.double()
    return float((got.double() - want).norm() / (want.norm() + 1e-300))


def _nhwc(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev, torch.float32)


def _nchw(t):
    return t.cpu().permute(0, 3, 1, 2)


@pytest.mark.parametrize("ks,stride,cin,cout,B,H,mode", [
    (3, 1, 64, 64, 3, 56, 0),      # fused 9-tap kernel, 1 row per step
    (3, 1, 128, 128, 4, 28, 0),    # 2 rows per step
    (3, 2, 64, 128, 3, 56, 0),     # stride 2 window
    (3, 1, 512, 512, 5, 7, 0),     # odd map, several images per slab
    (3, 1, 256, 256, 3, 14, 1),    # per-tap kernel forced (the path of rows that do not fit the fused plan)
    (1, 2, 64, 128, 3, 56, 0),     # downsample branch
    (1, 2, 256, 512, 4, 14, 0),
    (3, 1, 64, 64, 2, 72, 0),      # Wo > 64: falls back to the per-tap kernel by itself
])
def test_wgrad_kernels(dev, ks, stride, cin, cout, B, H, mode):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(ks * 100 + cin + H)
    x = torch.randn(B, cin, H, H, generator=g, dtype=torch.float64)
    w = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride, ks // 2)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, w, dz)
    dw = torch.empty(cout, cin, ks, ks, dtype=torch.float32, device=dev)
    xd, dzd = _nhwc(x, dev), _nhwc(dz, dev)
    check(lib().dh_debug_wgrad_f32(dzd.data_ptr(), xd.data_ptr(), dw.data_ptr(), B, H, H, cin, cout, ks, stride, mode, None), "wgrad")
    assert _rel(dw.cpu(), want) <= TOL
    # edge taps on their own: a wrong border would drown in the full-tensor norm of a large map
    if ks == 3:
        for t in ((0, 0), (0, 2), (2, 0), (2, 2)):
            assert _rel(dw.cpu()[:, :, t[0], t[1]], want[:, :, t[0], t[1]]) <= TOL, t


@pytest.mark.parametrize("B,P", [(3, 64), (2, 224)])
def test_stem_wgrad_kernel(dev, B, P):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(P)
    x = torch.rand(B, 3, P, P, generator=g, dtype=torch.float64)
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, 2, 3)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, w, dz)
    dw = torch.empty(64, 3, 7, 7, dtype=torch.float32, device=dev)
    xd = x.to(dev, torch.float32).contiguous()
    check(lib().dh_debug_stem_wgrad_f32(_nhwc(dz, dev).data_ptr(), xd.data_ptr(), dw.data_ptr(), B, P, None), "stem wgrad")
    assert _rel(dw.cpu(), want) <= TOL


@pytest.mark.parametrize("B,P", [(3, 64), (2, 224), (5, 96), (64, 224)])
def test_stem_wgrad_bf16_kernel(dev, B, P):
    """The bf16 engine's stem weight gradient (stem_wgrad_bf16_kernel: 16 output pixels per bf16 MFMA, x rounded to bf16 on its way into
    LDS) against float64 on the SAME bf16 operands: float32 accumulation of exact bf16 products, so 1e-5 relative; two runs equal bits."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(P + B)
    x = torch.rand(B, 3, P, P, generator=g)
    xb = x.bfloat16().double()
    w = torch.zeros(64, 3, 7, 7, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(xb, w, None, 2, 3)
    dz = torch.randn(y.shape, generator=g).bfloat16()
    (want,) = torch.autograd.grad(y, w, dz.double())
    xd = x.to(dev).contiguous()
    dzd = dz.permute(0, 2, 3, 1).contiguous().to(dev)
    outs = []
    for _ in range(2):
        dw = torch.empty(64, 3, 7, 7, dtype=torch.float32, device=dev)
        check(lib().dh_debug_stem_wgrad_bf16(dzd.data_ptr(), xd.data_ptr(), dw.data_ptr(), B, P, None), "stem wgrad bf16")
        outs.append(dw.cpu())
    assert torch.equal(outs[0], outs[1])
    assert _rel(outs[0], want) <= 1e-5


@pytest.mark.parametrize("ks,stride,cin,cout,B,H,res", [
    (3, 1, 64, 64, 2, 32, True), (3, 1, 256, 256, 3, 14, False), (3, 2, 64, 128, 2, 32, False),
    (3, 2, 256, 512, 3, 14, False), (1, 2, 64, 128, 2, 32, True), (1, 2, 256, 512, 3, 14, True),
    # the four parity classes of the stride-2 data gradient (round 3): odd maps (classes of unequal size), a joining gradient,
    # enough images for several tile rounds and for the 512-pixel tile variant
    (3, 2, 64, 128, 2, 15, False), (3, 2, 128, 256, 3, 7, True), (3, 2, 64, 128, 40, 56, True), (3, 2, 64, 64, 2, 9, False),
])
def test_dgrad_paths(dev, ks, stride, cin, cout, B, H, res):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(ks * 10 + stride + cin)
    x = torch.zeros(B, cin, H, H, dtype=torch.float64, requires_grad=True)
    w = torch.randn(cout, cin, ks, ks, generator=g, dtype=torch.float64) * (2.0 / (cin * ks * ks)) ** 0.5
    y = F.conv2d(x, w, None, stride, ks // 2)
    dz = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dz)
    r = torch.randn(B, cin, H, H, generator=g, dtype=torch.float64) if res else None
    if res:
        want = want + r
    dx = torch.empty(B, H, H, cin, dtype=torch.float32, device=dev)
    wd = w.to(dev, torch.float32).contiguous()
    rd = _nhwc(r, dev) if res else None
    check(lib().dh_debug_dgrad_f32(_nhwc(dz, dev).data_ptr(), wd.data_ptr(), rd.data_ptr() if res else None, dx.data_ptr(),
                                   B, H, H, cin, cout, ks, stride, None), "dgrad")
    assert _rel(_nchw(dx), want) <= TOL


@pytest.mark.parametrize("C,B,H,relu,res", [(64, 4, 28, True, False), (128, 3, 14, True, True), (512, 6, 7, False, False),
                                            (256, 2, 56, True, True), (64, 2, 8, 2, False)])
def test_bn_forward_backward_kernels(dev, C, B, H, relu, res):
    """relu: False / True (backward pattern read from y) / 2 (pattern recomputed from z: the engine's mode for every block's first BN;
    no residual, no masked gradient g -- 128 rows = eight reduce workgroups at C = 64)."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(C + H)
    z = (torch.randn(B, C, H, H, generator=g, dtype=torch.float64) * 1.7 + 0.4).requires_grad_(True)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    r = torch.randn(B, C, H, H, generator=g, dtype=torch.float64) if res else None
    rm, rv = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    pre = F.batch_norm(z, rm, rv, gamma, beta, True, 0.1, 1e-5)
    if res:
        pre = pre + r
    y = F.relu(pre) if relu else pre
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    dz_w, dg_w, db_w = torch.autograd.grad(y, (z, gamma, beta), dy)
    g_w = dy * (y > 0) if relu else dy
    rows = B * H * H
    zd, dyd = _nhwc(z.detach(), dev), _nhwc(dy, dev)
    yd, dzd, gd = torch.empty_like(zd), torch.empty_like(zd), torch.empty_like(zd)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    st = torch.empty(4 * C, device=dev)
    gmd, btd = gamma.detach().to(dev, torch.float32), beta.detach().to(dev, torch.float32)
    rd = _nhwc(r, dev) if res else None
    check(lib().dh_debug_bn_f32(zd.data_ptr(), gmd.data_ptr(), btd.data_ptr(), rd.data_ptr() if res else None, int(relu),
                                yd.data_ptr(), dyd.data_ptr(), dzd.data_ptr(), gd.data_ptr() if relu != 2 else None, dg.data_ptr(),
                                db.data_ptr(), st.data_ptr(), rows, C, None), "bn")
    if relu == 2:   # the same inputs with the pattern read from y: the recomputed pattern is bit-identical (comment at col_reduce_kernel)
        y1, dz1 = torch.empty_like(zd), torch.empty_like(zd)
        dg1, db1 = torch.empty_like(dg), torch.empty_like(db)
        check(lib().dh_debug_bn_f32(zd.data_ptr(), gmd.data_ptr(), btd.data_ptr(), None, 1, y1.data_ptr(), dyd.data_ptr(), dz1.data_ptr(),
                                    gd.data_ptr(), dg1.data_ptr(), db1.data_ptr(), None, rows, C, None), "bn relu=1")
        assert torch.equal(y1, yd) and torch.equal(dz1, dzd) and torch.equal(dg1, dg) and torch.equal(db1, db)
    assert _rel(_nchw(yd), y.detach()) <= TOL
    # the ReLU pattern of the float32 forward can differ from float64 where |pre-activation| ~ 1e-7: compare the backward
    # with torch's pattern imposed on the few such elements excluded (none in practice at these sizes)
    same_mask = (_nchw(yd) > 0) == (y.detach() > 0) if relu else torch.ones_like(y, dtype=torch.bool)
    assert float(same_mask.double().mean()) >= 0.99999
    assert _rel(_nchw(gd), g_w) <= TOL
    assert _rel(dg.cpu(), dg_w) <= TOL and _rel(db.cpu(), db_w) <= TOL
    assert _rel(_nchw(dzd), dz_w) <= 2 * TOL      # dz = k0 g + k1 z + k2: three rounded coefficients
    s = st.cpu().double()
    mean_w = z.detach().mean((0, 2, 3))
    var_w = z.detach().var((0, 2, 3), unbiased=False)
    assert _rel(s[:C], mean_w) <= TOL and _rel(s[C:2 * C], 1.0 / torch.sqrt(var_w + 1e-5)) <= TOL
    assert _rel(s[2 * C:3 * C], rm) <= TOL and _rel(s[3 * C:], rv) <= TOL     # momentum 0.1, unbiased variance (torch updated rm / rv in place)


@pytest.mark.parametrize("B,H,C", [(3, 112, 64), (2, 31, 64), (4, 16, 128)])
def test_maxpool_forward_backward_kernels(dev, B, H, C):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, C, H, H, generator=g)
    x[:, ::2] = (x[:, ::2] * 2).round() / 2     # half of the channels quantised: plenty of exact ties inside the 3x3 windows
    x = x.double().requires_grad_(True)
    y = F.max_pool2d(x, 3, 2, 1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    (want,) = torch.autograd.grad(y, x, dy)
    xd, dyd = _nhwc(x.detach(), dev), _nhwc(dy, dev)
    Ho = y.shape[2]
    yd = torch.empty(B, Ho, Ho, C, dtype=torch.float32, device=dev)
    dxd = torch.empty_like(xd)
    check(lib().dh_debug_maxpool_f32(xd.data_ptr(), yd.data_ptr(), dyd.data_ptr(), dxd.data_ptr(), B, H, H, C, None), "maxpool")
    assert torch.equal(_nchw(yd), y.detach().float())
    assert _rel(_nchw(dxd), want) <= 1e-6      # gradients are routed, not computed: only float32 sums of <= 4 terms


@pytest.mark.parametrize("B,H,C", [(3, 112, 64), (2, 31, 64), (4, 16, 128)])
def test_bn_pool_fused_stem_tail_f32(dev, B, H, C):
    """The float32 engine's fused stem tail (bn_apply_pool_kernel; bn_pool_bwd_reduce / _apply: the maxpool's gradient gathered inside the BN
    backward passes) against the unfused kernels it replaces -- pooled map bit for bit (the same float32 values are compared), dz / dgamma /
    dbeta to summation order -- and against float64 autograd through relu(bn(z)) and max_pool2d."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(H + C)
    z = (torch.randn(B, C, H, H, generator=g, dtype=torch.float64) * 1.3 + 0.2)
    z[:, ::2] = (z[:, ::2] * 2).round() / 2     # half of the channels quantised: exact ties inside the windows
    z.requires_grad_(True)
    gamma = (0.5 + torch.rand(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    beta = (0.1 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = F.relu(F.batch_norm(z, None, None, gamma, beta, True, 0.1, 1e-5))
    p = F.max_pool2d(y, 3, 2, 1)
    Hp = p.shape[2]
    dp = torch.randn(p.shape, generator=g, dtype=torch.float64)
    dz_w, dg_w, db_w = torch.autograd.grad(p, (z, gamma, beta), dp)
    zd, dpd = _nhwc(z.detach(), dev), _nhwc(dp, dev)
    gmd, btd = gamma.detach().to(dev, torch.float32), beta.detach().to(dev, torch.float32)
    pooled = torch.empty(B, Hp, Hp, C, dtype=torch.float32, device=dev)
    idx = torch.empty(B, Hp, Hp, C, dtype=torch.uint8, device=dev)
    dz = torch.empty_like(zd)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    check(lib().dh_debug_bn_pool_f32(zd.data_ptr(), gmd.data_ptr(), btd.data_ptr(), pooled.data_ptr(), idx.data_ptr(), dpd.data_ptr(), dz.data_ptr(),
                                     dg.data_ptr(), db.data_ptr(), B, H, H, C, None), "bn pool")
    # the unfused chain: BN apply -> maxpool forward / backward -> BN backward (mask from y)
    yd, dyd = torch.empty_like(zd), torch.empty_like(zd)
    p2 = torch.empty_like(pooled)
    dz2, g2 = torch.empty_like(zd), torch.empty_like(zd)
    dg2, db2 = torch.empty(C, device=dev), torch.empty(C, device=dev)
    check(lib().dh_debug_bn_f32(zd.data_ptr(), gmd.data_ptr(), btd.data_ptr(), None, 1, yd.data_ptr(), None, None, None, None, None, None,
                                B * H * H, C, None), "bn")
    check(lib().dh_debug_maxpool_f32(yd.data_ptr(), p2.data_ptr(), dpd.data_ptr(), dyd.data_ptr(), B, H, H, C, None), "maxpool")
    check(lib().dh_debug_bn_f32(zd.data_ptr(), gmd.data_ptr(), btd.data_ptr(), None, 1, yd.data_ptr(), dyd.data_ptr(), dz2.data_ptr(), g2.data_ptr(),
                                dg2.data_ptr(), db2.data_ptr(), None, B * H * H, C, None), "bn bwd")
    assert torch.equal(pooled, p2)
    assert _rel(dz.cpu(), dz2.cpu()) <= 1e-6 and _rel(dg.cpu(), dg2.cpu()) <= 1e-6 and _rel(db.cpu(), db2.cpu()) <= 1e-6
    # float64 reference
    assert _rel(_nchw(pooled), p.detach()) <= TOL
    assert _rel(dg.cpu(), dg_w) <= TOL and _rel(db.cpu(), db_w) <= TOL
    assert _rel(_nchw(dz), dz_w) <= 2 * TOL
    ii = idx.cpu().long()
    assert int(ii.max()) <= 8


# ---- bf16 engine (train2): the GEMM-shaped kernels on their own ------------------------------------------------------
def _bf(t):
    return t.bfloat16().float()


@pytest.mark.parametrize("M,N,K,stride", [(1000, 64, 64, 1), (3136, 256, 64, 1), (777, 128, 512, 1), (3136, 2048, 512, 1),
                                          (4 * 14 * 14, 512, 256, 2), (2 * 28 * 28, 128, 64, 2)])
def test_gemm1x1_bf16_kernel(dev, M, N, K, stride):
    """out = A . W^T (+ res) on bf16 MFMA with f32 accumulation against float64 on the same bf16 operands: the products are exact,
    only the output rounding to bf16 (2^-9 relative) and the f32 summation order remain."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(M + N + K)
    w = _bf(torch.randn(N, K, generator=g) * (1.0 / K) ** 0.5)
    res = _bf(torch.randn(M, N, generator=g))
    if stride == 1:
        a = _bf(torch.randn(M, K, generator=g))
        rows, geo = a, (1, 1, 1, 1)
    else:
        B, Ho = (4, 14) if K == 256 else (2, 28)
        full = _bf(torch.randn(B, 2 * Ho, 2 * Ho, K, generator=g))
        a, rows, geo = full, full[:, ::2, ::2, :].reshape(M, K), (Ho, Ho, 2 * Ho, 2 * Ho)
    want = rows.double() @ w.double().T + res.double()
    ad, wd, rd = a.to(dev).bfloat16().contiguous(), w.to(dev).bfloat16().contiguous(), res.to(dev).bfloat16().contiguous()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    check(lib().dh_debug_gemm1x1_bf16(ad.data_ptr(), wd.data_ptr(), rd.data_ptr(), out.data_ptr(), M, N, K, stride, *geo, 1, None), "gemm")
    got = out.float().cpu().double()
    assert float((got - want).abs().max()) <= 2 ** -8 * max(1.0, float(want.abs().max()))
    assert _rel(got, want) <= 3e-3
    # element by element: |got - round(want)| <= ulp + gamma_K A (oracle/layer_ref.py); the maximum above lets a small element be anything
    from oracle import layer_ref as lr
    A = rows.double().abs() @ w.double().abs().T + res.double().abs()
    ok = lr.gate_mask(got.numpy(), lr.round_to(want.numpy(), "bf16"), A.numpy(), lr.rounding_count(K, 1, "bf16", True), "bf16")
    bad = np.argwhere(~ok)
    assert ok.all(), f"{len(bad)} of {ok.size} elements outside the gate, first (row, channel) {bad[:8].tolist()}, rows {np.unique(bad[:, 0])[:16].tolist()}"


@pytest.mark.parametrize("ks,stride,cin,cout,B,H", [
    (3, 1, 64, 64, 3, 56), (3, 1, 256, 256, 4, 14), (3, 2, 128, 128, 3, 28), (3, 1, 512, 512, 5, 7), (3, 1, 128, 128, 2, 12),
    (1, 1, 64, 256, 3, 56), (1, 1, 256, 64, 2, 28),          # 64 x 64 tiles (64-channel layers)
    (1, 1, 512, 128, 3, 28), (1, 1, 256, 1024, 4, 14), (1, 1, 2048, 512, 5, 7), (1, 2, 256, 512, 3, 28), (1, 1, 1024, 256, 2, 6),   # 128 x 128 tiles
    (1, 1, 1024, 256, 64, 14), (1, 2, 512, 1024, 8, 28), (1, 1, 64, 256, 64, 56), (1, 1, 128, 128, 1, 5),   # round 4: ring kernel at bench shapes / many slabs / one partial step
])
def test_wgrad_bf16_kernels(dev, ks, stride, cin, cout, B, H):
    """dW through the transposed-LDS-read kernels (3x3 tap groups, 1x1 with 64 x 64 tiles, and -- round 4 -- the LDS-DMA ring kernel
    with four-quadrant tiles over flat 64-pixel steps, wgrad_ring.inc; odd maps, stride 2, a pixel count that is not a multiple of
    64, row pitches that are not multiples of 4) against torch autograd in float64 on the same bf16 operands: relative L2 <= 1e-5
    (exact products, f32 accumulation)."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(ks * 1000 + cin + cout + H)
    x = _bf(torch.randn(B, cin, H, H, generator=g)).double()
    w = torch.zeros(cout, cin, ks, ks, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(x, w, None, stride, ks // 2)
    dz = _bf(torch.randn(y.shape, generator=g)).double()
    (want,) = torch.autograd.grad(y, w, dz)
    xd = x.float().permute(0, 2, 3, 1).contiguous().to(dev).bfloat16()
    dzd = dz.float().permute(0, 2, 3, 1).contiguous().to(dev).bfloat16()
    dw = torch.empty(cout, cin, ks, ks, dtype=torch.float32, device=dev)
    check(lib().dh_debug_wgrad_bf16(dzd.data_ptr(), xd.data_ptr(), dw.data_ptr(), B, H, H, cin, cout, ks, stride, 1, None), "wgrad bf16")
    assert _rel(dw.cpu(), want) <= TOL
    if ks == 3:
        for t in ((0, 0), (0, 2), (2, 0), (2, 2), (1, 1)):
            assert _rel(dw.cpu()[:, :, t[0], t[1]], want[:, :, t[0], t[1]]) <= TOL, t


@pytest.mark.parametrize("M,N,K", [(777, 64, 64), (3136, 256, 1024), (12544, 128, 256), (128 * 129 + 5, 64, 128), (50176, 128, 64)])
def test_gemm1x1_fused_epilogues(dev, M, N, K):
    """The fused epilogues of the ring GEMM (gemm1x1.inc).  Statistics: mean / invstd of the bf16-ROUNDED output (what the BN of
    train.py's model normalises) against float64 over the kernel's own output: 1e-6 relative (f32 partials of <= 128 values,
    double column sums in the finalize launch).
    Mask: the output is zero exactly where the mask tensor is <= 0, and untouched elsewhere (bit-equal to the unmasked run).
    Repeating the launch gives the same bits."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(M + N + K)
    a = _bf(torch.randn(M, K, generator=g)).to(dev).bfloat16().contiguous()
    w = _bf(torch.randn(N, K, generator=g) * (1.0 / K) ** 0.5).to(dev).bfloat16().contiguous()
    res = _bf(torch.randn(M, N, generator=g)).to(dev).bfloat16().contiguous()
    msk = torch.relu(torch.randn(M, N, generator=g)).to(dev).bfloat16().contiguous()
    msk.view(-1)[::7] = -0.0     # a negative zero masks like a zero
    geo = (1, 1, 1, 1, 1)
    fn = lib().dh_debug_gemm1x1_fused_bf16
    plain = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    check(lib().dh_debug_gemm1x1_bf16(a.data_ptr(), w.data_ptr(), None, plain.data_ptr(), M, N, K, *geo, 1, None), "gemm")
    # statistics
    out = torch.empty_like(plain)
    mean = torch.empty(N, dtype=torch.float32, device=dev)
    invstd = torch.empty_like(mean)
    for rep in (1, 3):
        mean.fill_(float("nan")); invstd.fill_(float("nan"))
        check(fn(a.data_ptr(), w.data_ptr(), None, None, out.data_ptr(), mean.data_ptr(), invstd.data_ptr(), M, N, K, *geo, rep, None), "fused")
        assert torch.equal(out, plain)
        z = out.double()
        mu, var = z.mean(0), z.var(0, unbiased=False)
        assert float(((mean.double() - mu).abs() / (z.abs().mean(0) + 1e-12)).max()) <= 1e-6
        assert float((invstd.double() * torch.sqrt(var + 1e-5) - 1).abs().max()) <= 1e-6
        if rep == 1:
            first = (mean.clone(), invstd.clone())
        else:
            assert torch.equal(mean, first[0]) and torch.equal(invstd, first[1])
    # residual + mask
    both = torch.empty_like(plain)
    unmasked = torch.empty_like(plain)
    check(fn(a.data_ptr(), w.data_ptr(), res.data_ptr(), None, unmasked.data_ptr(), None, None, M, N, K, *geo, 1, None), "fused")
    check(fn(a.data_ptr(), w.data_ptr(), res.data_ptr(), msk.data_ptr(), both.data_ptr(), None, None, M, N, K, *geo, 1, None), "fused")
    keep = msk.float() > 0
    assert torch.equal(both[keep], unmasked[keep])
    assert int((both[~keep].view(torch.int16) != 0).sum()) == 0


# ---- bf16 engine: the HBM-bound kernels one by one ---------------------------------------------------
def _bf16_ulp_close(got, want64, slack=1.0):
    """`got` (bf16 tensor) equals float64 `want64` up to the final rounding to bf16: |err| <= slack * 2^-8 * |want| + tiny."""
    g = got.float().cpu().double()
    return bool(((g - want64).abs() <= slack * 2.0 ** -8 * want64.abs() + 1e-30).all())


@pytest.mark.parametrize("rows,C,relu,with_res,mode", [(3136, 64, 1, False, 2), (50176, 64, 1, False, 2), (784 * 3, 256, 1, True, 1),
                                                       (784 * 3, 256, 1, True, 0), (196 * 7 + 3, 1024, 0, False, 0), (49 * 5, 2048, 1, True, 1),
                                                       (200704, 128, 1, False, 2), (12544, 512, 1, True, 1)])
def test_bn2_bf16_kernels(dev, rows, C, relu, with_res, mode):
    """bf16 engine BN: statistics (per-workgroup partial sums + finalize launch), apply (+ identity)(+ ReLU), backward reduce + apply, against torch
    autograd in float64 on the same bf16 operands.  Saved mean / invstd and dgamma / dbeta (float32 results of double
    column sums in a fixed order): relative 1e-5.  y and dz are bf16: equal to the float64 result up to the final rounding (one bf16 ulp, 2^-8
    relative; dz: the coefficients are float32, so 2 ulp).  mode 0 = no mask in the backward kernels (dy pre-masked by the
    test, as the dgrad GEMM's epilogue does it in the engine), 1 = mask from y, 2 = mask recomputed from z.  Two runs: equal bits."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(rows + C + mode)
    z = _bf(torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g))
    res = _bf(torch.randn(rows, C, generator=g)) if with_res else None
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    dy = _bf(torch.randn(rows, C, generator=g) * 1e-3)
    z64 = z.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu, var = z64.mean(0), z64.var(0, unbiased=False)
    yb = (z64 - mu) / torch.sqrt(var + 1e-5) * g64 + b64
    if with_res:
        yb = yb + res.double()
    y64 = torch.relu(yb) if relu else yb
    zd = z.to(dev).bfloat16().contiguous()
    rd = res.to(dev).bfloat16().contiguous() if with_res else None
    gd, bd = gamma.to(dev), beta.to(dev)
    outs = []
    for _ in range(2):
        y = torch.empty(rows, C, dtype=torch.bfloat16, device=dev)
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty_like(mean)
        dz = torch.empty_like(y)
        gout = torch.empty_like(y) if mode == 1 else None
        dgam, dbet = torch.empty_like(mean), torch.empty_like(mean)
        if relu and mode == 0:     # the engine hands such a BN a gradient that is already masked
            dyd = (dy * (y64.detach() > 0).float()).to(dev).bfloat16().contiguous()
        else:
            dyd = dy.to(dev).bfloat16().contiguous()
        check(lib().dh_debug_bn2_bf16(zd.data_ptr(), rd.data_ptr() if with_res else None, gd.data_ptr(), bd.data_ptr(), relu, y.data_ptr(),
                                      mean.data_ptr(), invstd.data_ptr(), dyd.data_ptr(), mode if relu else 0, dz.data_ptr(),
                                      gout.data_ptr() if gout is not None else None, dgam.data_ptr(), dbet.data_ptr(), rows, C, None), "bn2")
        outs.append((y, mean, invstd, dz, dgam, dbet))
    for a, b in zip(*outs):
        assert torch.equal(a, b)                                            # fixed-order sums: no run-to-run difference
    y, mean, invstd, dz, dgam, dbet = outs[0]
    assert float((mean.cpu().double() - mu.detach()).abs().max()) <= 1e-6 * float(z.abs().max())
    assert float((invstd.cpu().double() * torch.sqrt(var.detach() + 1e-5) - 1).abs().max()) <= 1e-6
    # y: the engine normalises with float32 coefficients, then rounds to bf16
    yg = y.float().cpu().double()
    assert float((yg - y64.detach()).abs().max()) <= 2.0 ** -8 * float(y64.abs().max()) + 1e-6
    assert _rel(yg, y64.detach()) <= 3e-3
    # backward against autograd: dL = sum(y * dy)
    (y64 * dy.double()).sum().backward()
    assert _rel(dgam.cpu(), g64.grad) <= 1e-5 and _rel(dbet.cpu(), b64.grad) <= 1e-5
    dzg = dz.float().cpu().double()
    assert _rel(dzg, z64.grad) <= 3e-3
    if gout is not None:
        assert torch.equal(gout.float().cpu(), (dy * (y.float().cpu() > 0).float()))


@pytest.mark.parametrize("with_res,mode", [(True, 1), (False, 2)])
@pytest.mark.parametrize("rows", [1000, 16448])
def test_bn2_hook_equals_the_paths_hook(dev, rows, with_res, mode):
    """dh_debug_bn2_bf16 is dh_debug_bn2_paths_bf16 with the engine's default fold (1), no pattern bytes and no join: the same operands
    through both give the same bits in y, mean, invstd, dz, g_out, dgamma and dbeta.  C = 64; rows on either side of the DH_T2_FOLD_ROWS
    default of 16384 (a folded small map, and the finalize launch + elementwise pass); residual + ReLU pattern from y with the masked
    gradient written, and no residual + pattern recomputed from z."""
    from deephisto_amd._lib import check, lib
    C = 64
    g = torch.Generator().manual_seed(rows + mode)
    zd = (torch.randn(rows, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g)).to(dev).bfloat16()
    rd = torch.randn(rows, C, generator=g).to(dev).bfloat16() if with_res else None
    gd, bd = (torch.rand(C, generator=g) + 0.5).to(dev), (torch.randn(C, generator=g) * 0.3).to(dev)
    dyd = (torch.randn(rows, C, generator=g) * 1e-3).to(dev).bfloat16()
    ptr = lambda t: t.data_ptr() if t is not None else None

    def outputs():
        o = {k: torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=dev) for k in ("y", "dz")}
        o["g_out"] = torch.full((rows, C), float("nan"), dtype=torch.bfloat16, device=dev) if mode == 1 else None
        o.update({k: torch.full((C,), float("nan"), dtype=torch.float32, device=dev) for k in ("mean", "invstd", "dgamma", "dbeta")})
        return o

    a, b = outputs(), outputs()
    check(lib().dh_debug_bn2_bf16(ptr(zd), ptr(rd), ptr(gd), ptr(bd), 1, ptr(a["y"]), ptr(a["mean"]), ptr(a["invstd"]), ptr(dyd), mode,
                                  ptr(a["dz"]), ptr(a["g_out"]), ptr(a["dgamma"]), ptr(a["dbeta"]), rows, C, None), "bn2")
    check(lib().dh_debug_bn2_paths_bf16(ptr(zd), ptr(rd), ptr(gd), ptr(bd), 1, 1, ptr(b["y"]), None, ptr(b["mean"]), ptr(b["invstd"]),
                                        None, None, None, None, None, ptr(dyd), mode, ptr(b["dz"]), ptr(b["g_out"]), ptr(b["dgamma"]),
                                        ptr(b["dbeta"]), rows, C, None), "bn2 paths")
    for k, t in a.items():
        if t is not None:
            assert not bool(torch.isnan(t.float()).any()), k      # written in full
            assert torch.equal(t, b[k]), k


@pytest.mark.parametrize("B,H,C", [(3, 112, 64), (2, 57, 64), (5, 14, 128)])
def test_maxpool2_bf16_kernels(dev, B, H, C):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(B * H + C)
    x = _bf(torch.randn(B, C, H, H, generator=g))
    x[:, :, 1::7, 2::5] = x[:, :, 0:-1:7, 1:-1:5][:, :, :x[:, :, 1::7, 2::5].shape[2], :x[:, :, 1::7, 2::5].shape[3]]   # ties
    x64 = x.double().requires_grad_(True)
    y64 = F.max_pool2d(x64, 3, 2, 1)
    dy = _bf(torch.randn(y64.shape, generator=g))
    (y64 * dy.double()).sum().backward()
    xd = x.permute(0, 2, 3, 1).contiguous().to(dev).bfloat16()
    dyd = dy.permute(0, 2, 3, 1).contiguous().to(dev).bfloat16()
    Ho = y64.shape[2]
    y = torch.empty(B, Ho, Ho, C, dtype=torch.bfloat16, device=dev)
    dx = torch.empty(B, H, H, C, dtype=torch.bfloat16, device=dev)
    check(lib().dh_debug_maxpool2_bf16(xd.data_ptr(), y.data_ptr(), dyd.data_ptr(), dx.data_ptr(), B, H, H, C, None), "maxpool2")
    assert torch.equal(y.float().cpu().permute(0, 3, 1, 2), y64.detach().float())
    want = x64.grad            # sums of <= 4 bf16 terms, rounded to bf16 once
    got = dx.float().cpu().permute(0, 3, 1, 2).double()
    assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())
    assert _rel(got, want) <= 3e-3


@pytest.mark.parametrize("B,H,C", [(3, 112, 64), (2, 57, 64), (4, 30, 128)])
def test_bn2_pool_fused_stem_tail_bf16(dev, B, H, C):
    """The stem's tail of the bf16 engine in one pass each way: pooled = maxpool3x3/2(bf16(relu(bn(z)))) + first-maximum positions straight
    from z (bn2_apply_pool_kernel), and dz / dgamma / dbeta with the maxpool's gradient gathered inside the BN backward passes
    (bn2_pool_bwd_reduce / _apply).  Forward against float64: pooled values within one bf16 ulp, every recorded position holds its window's
    maximum (within that ulp).  Backward against float64 autograd of sum(relu(bn(z)) * dY), dY = the pooled gradient scattered to the
    recorded positions: dz within 2 bf16 ulp, dgamma / dbeta 1e-5.  Two runs: equal bits."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(B * H + C + 5)
    z = _bf(torch.randn(B, H, H, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g) * 0.5)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.3
    Hp = (H + 2 - 3) // 2 + 1
    dpool = _bf(torch.randn(B, Hp, Hp, C, generator=g) * 1e-3)
    z64 = z.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    mu, var = z64.mean((0, 1, 2)), z64.var((0, 1, 2), unbiased=False)
    y64 = torch.relu((z64 - mu) / torch.sqrt(var + 1e-5) * g64 + b64)                     # [B, H, H, C]
    p64 = F.max_pool2d(y64.detach().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    zd, gd, bd, dpd = z.to(dev).bfloat16().contiguous(), gamma.to(dev), beta.to(dev), dpool.to(dev).bfloat16().contiguous()
    outs = []
    for _ in range(2):
        pooled = torch.empty(B, Hp, Hp, C, dtype=torch.bfloat16, device=dev)
        idx = torch.empty(B, Hp, Hp, C, dtype=torch.uint8, device=dev)
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd, dgam, dbet = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        dz = torch.empty(B, H, H, C, dtype=torch.bfloat16, device=dev)
        check(lib().dh_debug_bn2_pool_bf16(zd.data_ptr(), gd.data_ptr(), bd.data_ptr(), pooled.data_ptr(), idx.data_ptr(), mean.data_ptr(),
                                           invstd.data_ptr(), dpd.data_ptr(), dz.data_ptr(), dgam.data_ptr(), dbet.data_ptr(), B, H, H, C, None),
              "bn2 pool")
        outs.append((pooled, idx, mean, invstd, dz, dgam, dbet))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    pooled, idx, mean, invstd, dz, dgam, dbet = outs[0]
    assert float((mean.cpu().double() - mu.detach()).abs().max()) <= 1e-6 * float(z.abs().max())
    assert float((invstd.cpu().double() * torch.sqrt(var.detach() + 1e-5) - 1).abs().max()) <= 1e-6
    ulp = 2.0 ** -8 * float(p64.abs().max()) + 1e-6
    assert float((pooled.float().cpu().double() - p64).abs().max()) <= ulp
    # recorded positions: inside the map, and the value there is the window's maximum
    ii = idx.cpu().long()
    bb, oy, ox, cc = torch.meshgrid(torch.arange(B), torch.arange(Hp), torch.arange(Hp), torch.arange(C), indexing="ij")
    iy, ix = 2 * oy + ii // 3 - 1, 2 * ox + ii % 3 - 1
    assert int(ii.max()) <= 8 and bool(((iy >= 0) & (iy < H) & (ix >= 0) & (ix < H)).all())
    at = y64.detach()[bb, iy, ix, cc]
    assert float((at - p64).abs().max()) <= ulp
    # backward: the pooled gradient scattered to those positions, then autograd through relu(bn(z))
    dY = torch.zeros(B, H, H, C, dtype=torch.float64)
    dY.index_put_((bb.reshape(-1), iy.reshape(-1), ix.reshape(-1), cc.reshape(-1)), dpool.double().reshape(-1), accumulate=True)
    (y64 * dY).sum().backward()
    assert _rel(dgam.cpu(), g64.grad) <= 1e-5 and _rel(dbet.cpu(), b64.grad) <= 1e-5
    got, want = dz.float().cpu().double(), z64.grad
    assert float((got - want).abs().max()) <= 2.0 ** -7 * float(want.abs().max())
    assert _rel(got, want) <= 3e-3


def test_upsample2_add_and_avgpool_fc_dgrad_bf16(dev):
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(77)
    B, Ho, Hi, C = 3, 14, 28, 256
    t = _bf(torch.randn(B, Ho, Ho, C, generator=g))
    dx0 = _bf(torch.randn(B, Hi, Hi, C, generator=g))
    dxd = dx0.to(dev).bfloat16().contiguous()
    td = t.to(dev).bfloat16().contiguous()
    check(lib().dh_debug_upsample2_add_bf16(td.data_ptr(), dxd.data_ptr(), B, Ho, Ho, Hi, Hi, C, None), "upsample2")
    want = dx0.clone()
    want[:, ::2, ::2, :] = _bf(want[:, ::2, ::2, :] + t)
    assert torch.equal(dxd.float().cpu(), want)
    # odd input size: Hi = 2 Ho - 1
    Hi2 = 2 * Ho - 1
    dx1 = _bf(torch.randn(B, Hi2, Hi2, C, generator=g))
    dxd = dx1.to(dev).bfloat16().contiguous()
    check(lib().dh_debug_upsample2_add_bf16(td.data_ptr(), dxd.data_ptr(), B, Ho, Ho, Hi2, Hi2, C, None), "upsample2")
    want = dx1.clone()
    want[:, ::2, ::2, :] = _bf(want[:, ::2, ::2, :] + t)
    assert torch.equal(dxd.float().cpu(), want)
    # average pool + fc backward
    B, HW, C, K = 5, 49, 2048, 5
    dl = torch.randn(B, K, generator=g) * 0.1
    w = torch.randn(K, C, generator=g) * 0.05
    dx = torch.empty(B, HW, C, dtype=torch.bfloat16, device=dev)
    dld, wd = dl.to(dev), w.to(dev)
    check(lib().dh_debug_avgpool_fc_dgrad2(dld.data_ptr(), wd.data_ptr(), dx.data_ptr(), B, HW, C, K, None), "avgpool fc")
    want = (dl.double() @ w.double() / HW)[:, None, :].expand(B, HW, C)
    got = dx.float().cpu().double()
    assert float((got - want).abs().max()) <= 2.0 ** -8 * float(want.abs().max())


@pytest.mark.parametrize("M,N,K,mode", [(777, 64, 256, 2), (3136, 256, 64, 0), (12544, 128, 512, 2), (50176 + 3, 256, 64, 0)])
def test_gemm1x1_fused_bn_backward_sums(dev, M, N, K, mode):
    """The dgrad GEMM's epilogue leaves the sums of the following BN backward (sum g, sum g xhat): against float64 over the kernel's
    own (bf16) output and the same z / mean / invstd: relative 1e-5.  mode 2: g = out where fma(z, scale, shift) > 0 (float32, as
    the apply kernels compute it); mode 0: g = out as stored (here masked by a ReLU-output tensor, the pre-masked join gradient)."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(M + N + K + mode)
    a = _bf(torch.randn(M, K, generator=g)).to(dev).bfloat16().contiguous()
    w = _bf(torch.randn(N, K, generator=g) * (1.0 / K) ** 0.5).to(dev).bfloat16().contiguous()
    res = _bf(torch.randn(M, N, generator=g)).to(dev).bfloat16().contiguous() if mode == 0 else None
    msk = torch.relu(torch.randn(M, N, generator=g)).to(dev).bfloat16().contiguous() if mode == 0 else None
    z = _bf(torch.randn(M, N, generator=g) * 1.5 + 0.3).to(dev).bfloat16().contiguous()
    mean = z.float().mean(0).contiguous()
    invstd = (1.0 / torch.sqrt(z.float().var(0, unbiased=False) + 1e-5)).contiguous()
    gamma = (torch.rand(N, generator=g) + 0.5).to(dev)
    beta = (torch.randn(N, generator=g) * 0.3).to(dev)
    scale = (gamma * invstd).contiguous()
    shift = (beta - mean * scale).contiguous()
    out = torch.empty(M, N, dtype=torch.bfloat16, device=dev)
    sums = torch.empty(2 * N, dtype=torch.float32, device=dev)
    check(lib().dh_debug_gemm1x1_bwdsums_bf16(a.data_ptr(), w.data_ptr(), res.data_ptr() if res is not None else None,
                                              msk.data_ptr() if msk is not None else None, out.data_ptr(), z.data_ptr(), mean.data_ptr(),
                                              invstd.data_ptr(), scale.data_ptr(), shift.data_ptr(), mode, sums.data_ptr(), M, N, K, None), "bwd sums")
    o = out.float()
    if mode == 2:
        o = o * (torch.addcmul(shift, z.float(), scale) > 0).float()      # fma(z, scale, shift) > 0 in float32
    xhat = (z.double() - mean.double()) * invstd.double()
    s1 = o.double().sum(0)
    s2 = (o.double() * xhat).sum(0)
    assert _rel(sums[:N].cpu(), s1.cpu()) <= 1e-5 and _rel(sums[N:].cpu(), s2.cpu()) <= 1e-5
    if mode == 0:
        assert int((out[msk.float() <= 0].view(torch.int16) != 0).sum()) == 0


@pytest.mark.parametrize("cout,cin", [(64, 64), (128, 64), (128, 128), (256, 128), (512, 256), (512, 512)])
def test_pack_f32_tiles_match_the_elementwise_form(dev, cout, cin):
    """The float32 step re-packs its 3x3 weights after every update with a sub-tile kernel (16 couts x 64 cins x 9 taps through LDS, round 5);
    both operators -- forward and flipped / transposed for the data gradient -- must equal the element-wise packer of the load path bit for bit."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(cout * 7 + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g).to(dev)
    outs = [torch.full((cout * cin * 9,), float("nan"), device=dev) for _ in range(4)]
    check(lib().dh_debug_pack_f32(w.data_ptr(), cout, cin, *[o.data_ptr() for o in outs], None), "dh_debug_pack_f32")
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert not torch.isnan(outs[0]).any() and not torch.isnan(outs[1]).any()


@pytest.mark.parametrize("cout,cin", [(64, 64), (128, 64), (128, 128), (256, 128), (512, 256), (512, 512)])
def test_pack_bf16_tiles_match_the_elementwise_form(dev, cout, cin):
    """The bf16 engine re-packs its 3x3 weights one 64 x 64 tile per workgroup through LDS: both bf16 operators must equal the element-wise
    packer of the load path bit for bit."""
    from deephisto_amd._lib import check, lib
    g = torch.Generator().manual_seed(cout * 11 + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g).to(dev)
    outs = [torch.full((cout * cin * 9,), 0x7FC0, dtype=torch.int16, device=dev) for _ in range(4)]
    check(lib().dh_debug_pack_bf16(w.data_ptr(), cout, cin, *[o.data_ptr() for o in outs], None), "dh_debug_pack_bf16")
    assert torch.equal(outs[0], outs[2]) and torch.equal(outs[1], outs[3])
    assert int((outs[0] == 0x7FC0).sum()) == 0 and int((outs[1] == 0x7FC0).sum()) == 0
    if (cout, cin) != (128, 64):
        return
    # ... and to ground truth, not only to each other: the packed operands decoded by the kernels that read them (dh_debug_conv_bf16, which
    # packs with the same kernel).  Image b of a one-hot batch holds a single 1.0 at the centre of a 5 x 5 map in channel b, so every
    # output is one weight times one (exact) plus zeros.  Forward: Z[b][co] around the centre is w[co][b] flipped; data gradient:
    # dX[b][ci] around the centre is w[b][ci] as it stands -- the flipped and transposed operand undoes the forward's flip.
    wb = w.bfloat16().view(torch.int16).cpu()
    for dgrad, n_in, n_out in ((0, cin, cout), (1, cout, cin)):
        hot = torch.zeros(n_in, 5, 5, n_in, dtype=torch.bfloat16, device=dev)
        b = torch.arange(n_in, device=dev)
        hot[b, 2, 2, b] = 1.0
        out = torch.full((n_in, 5, 5, n_out), 0x7FC0, dtype=torch.int16, device=dev)
        check(lib().dh_debug_conv_bf16(hot.data_ptr(), w.data_ptr(), None, out.data_ptr(), n_in, 5, 5, cin, cout, 3, 1, dgrad, None), "one-hot conv")
        got = out.cpu()[:, 1:4, 1:4, :]                                   # [b][y][x][channel]
        if dgrad:
            want = wb.permute(0, 2, 3, 1)                                 # [co = b][ky][kx][ci]
        else:
            want = wb.flip(2, 3).permute(1, 2, 3, 0)                      # [ci = b][2 - ky][2 - kx][co]
        assert torch.equal(got, want), ("dgrad" if dgrad else "forward", int((got != want).sum()))
        ring = out.cpu().clone()
        ring[:, 1:4, 1:4, :] = 0
        assert int((ring & 0x7FFF).abs().sum()) == 0, "weights leaked outside the 3 x 3 neighbourhood"
