"""GPU: ONE convolution of the bf16 training engine at a time -- forward, 3x3 and 1x1 data gradient -- element by element against the
float64 reference (oracle/layer_ref.py: conv_epilogue, conv_dgrad), through dh_debug_conv_bf16, which packs the operands with the
step's packer and dispatches through the step's own t2_conv_fwd / t2_conv_dgrad.

The whole-network tests see these kernels through a relative L2 of 2e-2 per parameter tensor, which a wrong border row, a wrong
parity-class offset on a ragged tile or an image dropped from a partial image group does not move.  Here every element of every
referenced image must satisfy

    |got - want| <= ulp(want) + gamma_K * A          (want: the exact value rounded once to bf16; A, K: oracle/layer_ref.py)

at least IDENTICAL of them must equal the reference bit for bit, and two runs into NaN-prefilled outputs must give the same bits and
leave no prefill behind.  The strided 1x1 data gradient stores its low-resolution product before adding it into dX: its gate carries
the half ulp of that product (lr.stored_product_gate_mask, derived there), and its identical fraction is taken against the float64
value of those two stored roundings.  The cases (oracle/train_conv_cases.py) are the smallest shapes that reach each branch of the
CLS == 4 candidate table of plan_dgrad_s2 (csrc/conv3_plan_host.h) (16x16x1 / 8x8x2 / 8x8x4 tiles, MT 1 and 2, ragged tiles, an odd batch, a last group of one
image), each stride-1 tile variant up to the persistent 512-pixel one (tests/test_layer_reference_host.py checks that against
pick_stride1), the non-downsample stride-2 forward variant, and the 1x1 GEMM paths.  Batches above 16 images are referenced on a
selection (train_conv_cases.select); the other images are held to bit-equality between the two runs.
tests/test_layer_reference_host.py shows on the CPU that the gate fails every planted kernel error and that a float32 evaluation of
the same operands meets the floor on every case.

Measured figures (per case: the lowest identical fraction, the largest |got - want| / gate; the file's wall time) are NOT recorded yet:
this module has not run on an MI355X.  The test prints both figures per case (pytest -s) before it asserts; they are recorded here
only, and no threshold is derived from them.
"""
import numpy as np
import pytest
import torch

from oracle import train_conv_cases as tc

pytestmark = pytest.mark.gpu

IDENTICAL = 0.999      # the project's floor for bf16 storage (tests/test_gpu_layer_parity.py: IDENTICAL["bf16"])
PREFILL = 0x7FC0       # a bf16 NaN no kernel produces from finite operands


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _nhwc_bf16(t, dev):
    return t.permute(0, 2, 3, 1).contiguous().to(dev).bfloat16()


def _run(c, o, dev):
    """dh_debug_conv_bf16 twice into prefilled outputs: the bf16 bits of both runs, NHWC, on the device."""
    from deephisto_amd._lib import check, lib
    ind, wd = _nhwc_bf16(o.inp, dev), o.w.to(dev).contiguous()
    rd = _nhwc_bf16(o.res, dev) if o.res is not None else None
    shape = (c.B, c.H, c.H, c.cin) if c.dgrad else (c.B, c.Ho, c.Ho, c.cout)
    outs = []
    for _ in range(2):
        out = torch.full(shape, PREFILL, dtype=torch.int16, device=dev)
        check(lib().dh_debug_conv_bf16(ind.data_ptr(), wd.data_ptr(), rd.data_ptr() if rd is not None else None, out.data_ptr(),
                                       c.B, c.H, c.H, c.cin, c.cout, c.ks, c.stride, c.dgrad, None), f"dh_debug_conv_bf16 {c.name}")
        outs.append(out)
    return outs


def _fail_report(name, got, want, A, ok, sel):
    bad = np.argwhere(~ok)
    lines = [f"{name}: {len(bad)} of {ok.size} elements outside the gate; first (image, channel, y, x): got / want / A"]
    for i, ch, y, x in bad[:8]:
        lines.append(f"  image {int(sel[i])} c{ch} ({y},{x}): {got[i, ch, y, x]!r} / {want[i, ch, y, x]!r} / {A[i, ch, y, x]:.3g}")
    chans = np.unique(bad[:, 1])
    lines.append(f"  images {sorted(set(int(sel[i]) for i in bad[:, 0]))[:16]}, channels {chans[:16].tolist()} ({len(chans)}), "
                 f"rows {np.unique(bad[:, 2])[:16].tolist()}, cols {np.unique(bad[:, 3])[:16].tolist()}")
    return "\n".join(lines)


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_one_convolution_matches_float64_reference(dev, name):
    c = tc.BY_NAME[name]
    o = tc.operands(name)
    ref = tc.reference(name)
    first, second = _run(c, o, dev)
    assert torch.equal(first, second), f"{name}: two runs differ in {int((first != second).sum())} elements"
    assert int((first == PREFILL).sum()) == 0, f"{name}: {int((first == PREFILL).sum())} elements never written"
    sel = torch.from_numpy(ref.sel).to(dev)
    got = first[sel].view(torch.bfloat16).permute(0, 3, 1, 2).double().cpu().numpy()
    assert got.shape == ref.want.shape, name
    ok = tc.gate(c, ref, got)
    ratio = np.abs(got - ref.want) / _gate_width(c, ref)
    frac = float((got == ref.stored).mean())
    print(f"\n{name}: {len(ref.sel)} of {c.B} images, identical fraction {frac:.5f}, largest |got - want| / gate {ratio.max():.3f}")
    assert ok.all(), _fail_report(name, got, ref.want, ref.A, ok, ref.sel)
    assert frac >= IDENTICAL, f"{name}: only {frac:.5f} of the elements identical to the reference"


def _gate_width(c, ref):
    """The right-hand side of the gate (for the recorded ratio only; the assertion goes through tc.gate)."""
    from oracle import layer_ref as lr
    width = lr.quantum(ref.want, "bf16") + lr.gamma(ref.K) * ref.A
    if c.accumulate:
        width = width + 0.5 * lr.quantum(np.abs(ref.prod) + lr.gamma(ref.K) * ref.A_prod, "bf16")
    return width


def test_hook_refuses_what_the_engine_cannot_produce(dev):
    """Arguments outside the engine's reach are refused before any launch, and the message names the argument."""
    from deephisto_amd._lib import lib
    x = torch.zeros(2 * 16 * 16 * 128, dtype=torch.int16, device=dev)
    w = torch.zeros(128 * 128 * 9, dtype=torch.float32, device=dev)
    out = torch.zeros_like(x)

    def call(B=2, Hi=8, Wi=8, cin=64, cout=64, ks=3, stride=1, dgrad=1, res=None):
        return lib().dh_debug_conv_bf16(x.data_ptr(), w.data_ptr(), res, out.data_ptr(), B, Hi, Wi, cin, cout, ks, stride, dgrad, None)

    for kwargs, word in ((dict(ks=5), b"ks"), (dict(ks=2), b"ks"), (dict(stride=3), b"stride"), (dict(stride=0), b"stride"),
                         (dict(cin=96), b"cin"), (dict(cout=32), b"cout"), (dict(stride=2, Hi=7), b"Hi"), (dict(stride=2, Wi=7), b"Wi"),
                         (dict(ks=1, stride=2, Hi=7, Wi=7), b"Hi"), (dict(dgrad=0, res=x.data_ptr()), b"res"), (dict(dgrad=2), b"dgrad")):
        assert call(**kwargs) == -22, kwargs
        assert word in lib().dh_last_error(), (kwargs, lib().dh_last_error())
    assert call() == 0 and call(stride=2) == 0 and call(ks=1, stride=2, res=x.data_ptr()) == 0
