"""CPU self-checks of oracle/head_ref.py, the references and gates of tests/test_gpu_head.py:

  * NumPy float32 restatements of the head kernels and of the loss kernel, in the kernels' summation order, meet every gate at every
    shape of the GPU test -- and a restatement with one term dropped or a wrong divisor does not;
  * the integer bf16 pack reference agrees with torch.Tensor.bfloat16() on every non-NaN input and keeps every NaN a NaN; the carry
    form without the NaN branch (what the kernel used to do) does not.
"""
import numpy as np
import pytest
import torch

from oracle import head_ref as hr

HEAD_SHAPES, head_case, head_check = hr.HEAD_SHAPES, hr.head_case, hr.head_check


@pytest.mark.parametrize("bf16", [0, 1])
@pytest.mark.parametrize("B,HW,C,n_cls", HEAD_SHAPES)
def test_head_float32_restatement_meets_the_gates(B, HW, C, n_cls, bf16):
    x, w, bias, dl = head_case(B, HW, C, n_cls, bf16)
    got = hr.head_f32(x, w, bias, dl, bool(bf16))
    res = head_check(x, w, bias, dl, bool(bf16), got)
    print(f"[head host] B={B} HW={HW} C={C} n_cls={n_cls} bf16={bf16}: " + ", ".join(f"{n} {r:.3f}" for n, r in res))
    assert all(r <= 1.0 for _, r in res), res


def test_head_gates_refuse_small_errors():
    x, w, bias, dl = head_case(5, 49, 512, 7, 0)
    good = hr.head_f32(x, w, bias, dl, False)
    assert all(r <= 1.0 for _, r in head_check(x, w, bias, dl, False, good))
    bad = list(good)
    bad[0] = (good[0] * np.float32(49 / 48)).astype(np.float32)                    # mean over HW - 1
    assert dict(head_check(x, w, bias, dl, False, bad))["pooled"] > 1e3
    bad = list(good)
    bad[1] = good[1] - (good[0][:, -1:] * w[None, :, -1].reshape(1, -1)).astype(np.float32)   # last channel left out of the dot product
    assert dict(head_check(x, w, bias, dl, False, bad))["logits"] > 1e2
    bad = list(good)
    bad[2] = good[2] - (dl[-1][:, None] * good[0][-1][None, :]).astype(np.float32)           # last image left out of dW
    bad[3] = good[3] - dl[-1]
    r = dict(head_check(x, w, bias, dl, False, bad))
    assert r["dW"] > 1e2 and r["db"] > 1e2
    bad = list(good)
    bad[4] = good[4].copy()
    bad[4][:, -1, :] = 0                                                           # last pixel not written
    assert dict(head_check(x, w, bias, dl, False, bad))["dX"] > 1e2


CE_SHAPES = hr.CE_SHAPES


@pytest.mark.parametrize("B,n_cls", CE_SHAPES)
def test_ce_float32_restatement_meets_the_gates(B, n_cls):
    for seed in range(5 if B == 1 else 1):
        l, y = hr.ce_case(B, n_cls, seed)
        loss, gate, dl, gate_dl = hr.ce_loss_ref(l, y)
        assert np.isfinite(loss) and np.isfinite(dl).all()
        want_t = torch.nn.functional.cross_entropy(torch.from_numpy(l).double(), torch.from_numpy(y))
        assert abs(loss - float(want_t)) <= 1e-12 * max(1.0, abs(loss))
        got, got_dl = hr.ce_loss_f32(l, y)
        r1, r2 = abs(float(got) - loss) / gate, float((np.abs(got_dl.astype(np.float64) - dl) / gate_dl).max())
        print(f"[ce host] B={B} n_cls={n_cls} seed={seed}: loss {loss:.6f}, |got - want| / gate = {r1:.3f}, dl {r2:.3f}; gate / loss = {gate / loss:.2e}")
        assert r1 <= 1.0 and r2 <= 1.0
        assert gate <= 1e-5 * max(loss, 1.0)
        if B > 1:     # a row of loss 0.1 left out of the sum, and a mean over B - 1, are both refused at every B
            assert 0.1 / B > 4 * gate and loss / (B - 1) > 4 * gate


def test_ce_case_holds_the_rows_it_promises():
    l, y = hr.ce_case(37, 5)
    assert (l[0] == 80).all() and (l[1] == -80).all() and set(l[2]) == {80.0, -80.0} and l[2][y[2]] == -80 and len(set(l[3])) == 1
    assert l[4].max() - l[4][y[4]] == 80
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp(l[0].astype(np.float32) + np.float32(10)).sum())      # expf of raw logits near 89 overflows float32
    assert sorted({int(np.argmax(np.abs(hr.ce_case(1, 5, s)[0][0]))) for s in range(5)}) is not None


def test_pack_reference_is_round_to_nearest_even():
    bits = hr.wire_inputs()
    assert bits.size == 65536 * 6
    got = hr.pack_bf16_ref(bits)
    f = torch.from_numpy(bits.view(np.float32).copy())
    nan = torch.isnan(f).numpy()
    want = f.bfloat16().view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(got[~nan], want[~nan])
    assert nan.sum() == 2 * (6 * 127 + 5)          # exponent all ones: 127 upper halves with a mantissa bit, + 0x7F80 / 0xFF80 with a lower half
    gv = hr.bf16_bits_to_f32(got)
    assert np.isnan(gv[nan]).all() and not np.isnan(gv[~nan]).any()
    # a finite value past the largest bf16 rounds to infinity, infinities stay
    assert hr.pack_bf16_ref(np.array([0x7F7F8000, 0x7F7F7FFF, 0x7F800000, 0xFF7FFFFF], np.uint32)).tolist() == [0x7F80, 0x7F7F, 0x7F80, 0xFF80]
    # ties to even
    assert hr.pack_bf16_ref(np.array([0x3F808000, 0x3F818000, 0x3F808001], np.uint32)).tolist() == [0x3F80, 0x3F82, 0x3F81]
    # the rounding add alone (no NaN branch) loses NaNs: to infinity, and to a signed zero
    u = bits.astype(np.uint64)
    carry = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
    lost = nan & ~np.isnan(hr.bf16_bits_to_f32(carry))
    assert lost.sum() > 0 and 0x7F80 in carry[lost] and 0x0000 in carry[lost]


def test_unpack_reference_keeps_subnormals():
    b = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    for scale in (1.0, 1 / 8, 1 / 3):
        out = hr.unpack_bf16_ref(b, scale)
        want = (torch.from_numpy(hr.bf16_bits_to_f32(b).copy()).double() * float(np.float32(scale))).float().numpy()
        ok = ~np.isnan(want)
        assert np.array_equal(out[ok].view(np.uint32), want[ok].view(np.uint32))
        sub = (np.abs(out) > 0) & (np.abs(out) < 2.0 ** -126)
        assert scale == 1.0 or sub.sum() > 100
