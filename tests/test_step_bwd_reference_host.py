"""CPU: the judge of a whole step's backward pass (oracle/step_bwd_ref.py, used on the engine by tests/test_gpu_step_bwd.py) earns its trust
here, the way tests/test_bn_reference_host.py and tests/test_layer_reference_host.py do for theirs: a float32 evaluation of one training step
with the engine's bf16 stores and routes (`emulate_step`: ResNet-50, B = 3, P = 64 -- layer 1 has pre-masked blocks with in_mask and
epilogue sums, layer 2 maps of 192 rows = one and a half GEMM tiles, a stride-1 and three stride-2 downsample blocks) passes every gate on
every BN, inside the caps on undecided elements; and each of six errors planted INSIDE the pass, one at a time, is rejected -- at the
hand-off it breaks, by name.
"""
import functools

import pytest
import torch

from oracle import bn_ref as br
from oracle import resnet50 as o50
from oracle import step_bwd_ref as sb

B, P = 3, 64


@functools.lru_cache(maxsize=None)
def _reports(plant):
    model = o50.seeded_model(5, 5, perturb_bn=True).train()
    g = torch.Generator().manual_seed(1000 * B + P)
    x = torch.rand(B, 3, P, P, generator=g)
    labels = torch.randint(0, 5, (B,), generator=g)
    with torch.no_grad():
        s = sb.emulate_step(model, x, labels, plant)
    return s, sb.judge_step(s)


def _failures(reps):
    return [f for r in reps for f in r.failures]


def test_clean_emulation_passes_every_gate_on_every_bn():
    s, reps = _reports(None)
    assert not _failures(reps), "\n".join(_failures(reps))
    names = {r.name for r in reps}
    for L in s["topo"][1:]:
        assert f"{L['name']} BN backward" in names and f"{L['name']} route" in names, L["name"]
    assert "conv1 stem tail" in names and "conv1 grad_in" in names
    tops = [b["top"] for b in sb.blocks(s["topo"])]
    assert all(f"{t} grad_in" in names or f"{t} grad_in (head)" in names for t in tops)
    # inside the caps: the conditions of the GPU test are met by a correct float32 evaluation
    for r in reps:
        assert r.figures.get("undecided share", 0.0) <= br.UNDECIDED_CAP, r.line()
        assert r.figures.get("undecided windows", 0.0) <= br.WINDOW_CAP, r.line()
    fig = sb.figures(reps)
    print("\n[step bwd host] " + ", ".join(f"{k} {v[0]:.4g} ({v[1]})" for k, v in fig.items()))
    assert fig["dz identical"][0] >= sb.IDENTICAL and fig["grad_in identical"][0] >= sb.IDENTICAL


def test_the_emulation_takes_every_route_the_planted_errors_need():
    s, _ = _reports(None)
    routes = {n: t["route"] for n, t in s["tap"].items()}
    assert {r[sb.R_RELU] for r in routes.values()} == {0, 1, 2}
    assert any(r[sb.R_PREMASKED] and r[sb.R_HAVE_ROWS] > 0 and r[sb.R_RELU] == 0 for r in routes.values())      # top_rows
    assert any(r[sb.R_IN_MASK] for r in routes.values()) and any(r[sb.R_BRANCH] == 2 for r in routes.values())
    assert routes["layer2.1.conv3"][sb.R_HAVE_ROWS] == 2 and s["Z"]["layer2.1.conv3"][:, 0].size == 192     # a partial last tile


@pytest.mark.parametrize("arch,Bc,Pc,draw", sb.STEP_CASES)
def test_gpu_case_inputs_meet_the_window_cap(arch, Bc, Pc, draw):
    """A condition of the stem-tail reference, judged on the inputs alone (oracle/step_bwd_ref.py, STEP_CASES): the chosen draw is the
    first one under the cap."""
    from oracle import resnet18 as o18
    model = (o50 if arch == "resnet50" else o18).seeded_model(sb.STEP_SEED[arch], 5, perturb_bn=True)
    shares = [sb.stem_window_share(model, sb.case_inputs(Bc, Pc, d)[0]) for d in range(draw + 1)]
    print(f"\n[step bwd host] {arch} B={Bc} P={Pc}: undecided windows per draw {[round(v, 5) for v in shares]}")
    assert shares[-1] <= br.WINDOW_CAP and all(v > br.WINDOW_CAP for v in shares[:-1])


# plant -> (the report that must fail, a word of its failure)
PLANTED = {
    "identity_dropped_13_rows": ("layer1.0.conv3 grad_in", "grad_in"),
    "in_mask_of_the_block_before": ("layer1.1.conv3 grad_in", "grad_in"),
    "epilogue_sums_miss_last_tile": ("layer2.1.conv3 BN backward", "dgamma"),
    "stale_dy": ("layer1.1.conv1 grad_in", "grad_in"),
    "ds_product_not_rounded": ("layer1.2.conv3 grad_in", "identical"),
    "g_out_masked_by_z": ("layer1.2.conv3 g_out", "g_out"),
}


@pytest.mark.parametrize("plant", sb.PLANTS)
def test_planted_error_is_rejected_at_its_hand_off(plant):
    _, reps = _reports(plant)
    where, word = PLANTED[plant]
    rep = next(r for r in reps if r.name == where)
    assert any(word in f for f in rep.failures), f"{plant}: {where} passed\n{rep.line()}\n" + "\n".join(_failures(reps))
    if plant == "identity_dropped_13_rows":     # 13 pixels of the last image and nothing else
        assert rep.figures["grad_in outside"] <= 13 / (B * 16 * 16), rep.line()
    if plant == "ds_product_not_rounded":       # inside the element gate: only the value the stored roundings define tells
        assert rep.figures["grad_in outside"] == 0.0, rep.line()
