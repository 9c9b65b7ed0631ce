"""CPU self-check of oracle/bn_state_ref.py (the reference and gates of tests/test_gpu_bn_state.py): a float32 restatement of the engine's
running-statistics arithmetic meets the gates at the maps of the GPU test (n = 8 and 12 rows of the layer-4 maps up to the stem's 3072),
and the errors the suite could not see before do not: a biased variance (no n / (n - 1): 14 % at n = 8), a wrong momentum.  The eval-mode
restatement meets its gate with and without an identity and at a downsample join."""
import numpy as np
import pytest

from oracle import bn_state_ref as br
from oracle.head_ref import bf16_bits_to_f32, pack_bf16_ref


def _bf(a):
    return bf16_bits_to_f32(pack_bf16_ref(np.ascontiguousarray(a, np.float32).view(np.uint32)))


def _case(n, C, seed):
    rng = np.random.default_rng(seed + n + C)
    z = _bf(rng.standard_normal((n, C)) * (rng.random(C) + 0.5) + rng.standard_normal(C))
    return z, (0.1 * rng.standard_normal(C)).astype(np.float32), (0.5 + rng.random(C)).astype(np.float32), rng


@pytest.mark.parametrize("n,C,path,tile", [(8, 512, "cs", 1), (12, 2048, "gemm", 128), (32, 256, "cs", 1), (48, 1024, "gemm", 128),
                                           (128, 128, "cs", 4), (768, 64, "cs", 24), (2048, 64, "stats", 64), (3072, 64, "stats", 96)])
def test_running_update_restatement_and_planted_errors(n, C, path, tile):
    z, rm, rv, _ = _case(n, C, 1)
    K = br.chain_length(path, n, C)
    assert K >= min(n, tile)                     # the gate's chain is never shorter than the restatement's
    want_m, gate_m, want_v, gate_v = br.running_update_ref(z, rm, rv, K)
    got_m, got_v = br.running_update_f32(z, rm, rv, tile)
    r = (float((np.abs(got_m - want_m) / gate_m).max()), float((np.abs(got_v - want_v) / gate_v).max()))
    print(f"[bn host] n={n} C={C} {path} K={K}: |got - want| / gate = mean {r[0]:.3f}, var {r[1]:.3f}; gate / |want|: "
          f"{float((gate_m / np.abs(want_m).clip(1e-3)).max()):.1e}, {float((gate_v / want_v).max()):.1e}")
    assert r[0] <= 1.0 and r[1] <= 1.0
    _, bad_v = br.running_update_f32(z, rm, rv, tile, biased=True)
    assert float((np.abs(bad_v - want_v) > gate_v).mean()) > 0.99          # every channel shows the missing n / (n - 1), up to n = 3072
    bad_m, bad_v = br.running_update_f32(z, rm, rv, tile, momentum=0.01)
    assert float((np.abs(bad_m - want_m) > gate_m).mean()) > 0.95 and float((np.abs(bad_v - want_v) > gate_v).mean()) > 0.95


@pytest.mark.parametrize("kind", ["plain", "identity", "join", "no-relu"])
def test_eval_restatement_meets_the_gate(kind):
    n, C = 48, 256
    z, rm, rv, rng = _case(n, C, 7)
    gam, beta = (0.5 + rng.random(C)).astype(np.float32), (0.1 * rng.standard_normal(C)).astype(np.float32)
    s, h = br.eval_coefficients(gam, beta, rm, rv)
    idt = _bf(np.maximum(rng.standard_normal((n, C)), 0)) if kind == "identity" else None
    join = None
    if kind == "join":
        z2 = _bf(rng.standard_normal((n, C)) * 2)
        join = (z2, *br.eval_coefficients(gam[::-1].copy(), beta[::-1].copy(), rm[::-1].copy(), rv[::-1].copy()))
    relu = kind != "no-relu"
    want, gate = br.eval_y_ref(z, s, h, idt, relu, join)
    got = br.eval_y_f32(z, s, h, idt, relu, join)
    r = float((np.abs(got - want) / gate).max())
    print(f"[bn host] eval {kind}: worst |got - want| / gate = {r:.3f}")
    assert r <= 1.0
    # coefficients from the batch statistics of z instead of the running ones are refused
    s_b, h_b = br.eval_coefficients(gam, beta, z.mean(0), z.var(0))
    assert float((np.abs(br.eval_y_f32(z, s_b, h_b, idt, relu, join) - want) > gate).mean()) > 0.5
