"""GPU: the dZ chain and the BN gradients of a bf16 training step, as the step computes them, element by element against float64 from exactly
the operands the engine read (oracle/step_bwd_ref.py; the judge, a float32 emulation of the pass and six planted errors it rejects:
tests/test_step_bwd_reference_host.py).

tests/test_gpu_step_wgrad.py holds every conv weight gradient and every stored Z of a step; the kernels have float64 tests through their debug
hooks.  What neither sees is the host code between the kernels, t2_backward (csrc/train2.inc): six rotating gradient buffers, pre-masked
blocks (in_mask = the ReLU bits of ANOTHER block), BN-backward sums left in t->partial by a dgrad GEMM's epilogue and carried into the next
block (top_rows), two reduce / apply routes, the downsample branch accumulating into dX, the stem tail that never materialises dY.  A mask
taken from the wrong block or an identity gradient dropped on one ragged tile moves a few rows: far inside the 2e-2 / 6e-2 relative-L2 gates
of tests/test_gpu_train_bf16.py.  dh_train2_debug_backward_tap runs that same host code and copies out, for one BN per call, the gradient its
backward read (grad_in), the masked gradient it wrote (g_out), the statistics it read and the route it took; one forward and one tapped
backward per BN (a tapped backward follows a forward of its own), then per case:

  (a) BN backward     every BN, downsample BNs included: the dZ tap and p.grad of the BN's weight and bias against float64 BN backward of
                      grad_in on Z, the engine's mean / invstd and gamma, the ReLU pattern taken the way the recorded mode says
  (b) dgrad, joins    every grad_in against the float64 dgrad of the dZ tap above it (+ the identity gradient, * in_mask, + the downsample
                      product with its stored roundings); g_out == grad_in * (Y > 0) bit for bit; the last block's grad_in against the head
  (c) stem tail       conv1's dZ, dgamma, dbeta against the pool reference on the tapped pooled gradient
  (d) read-only       the gradient arena after EVERY tapped backward and every dZ bit-identical to an untapped step (m.train(), forward,
                      cross entropy, loss.backward()) from the same state
  (e) refusals        an unknown name, a wrong n_elem, g_out where no masked gradient is written, a null argument, no forward since the last
                      backward: -22, dh_last_error() names the argument
and across the cases the union of the route records holds every route of t2_backward (test_every_route_of_t2_backward_is_reached).
Gates, caps and exemptions: oracle/step_bwd_ref.py; none is set here.

Cases (oracle.step_bwd_ref.STEP_CASES): the four bf16 cases of tests/test_gpu_step_wgrad.py with its seeds, and ResNet-50 B = 29 P = 96: layer 1's map has 29 * 24 * 24 =
16 704 rows, the smallest batch above the fold limit of 16 384 (28 * 576 = 16 128), so its BNs take bn2_bwd_reduce_kernel and the finalize +
apply route, conv2's with 131 rows of epilogue sums (above the 128 the fold accepts), and 16 704 = 130 * 128 + 64 ends in a partial GEMM
tile.  Its float64 references cover images 0, 14, 27, 28 (the last holds the partial tile); the channel sums use every image, and every
tapped tensor of every image is held to bit-equality between two tapped runs.  Its images are the second seeded draw: the first does not
meet the stem reference's cap on undecided pool windows, a property of the inputs (STEP_CASES; tests/test_step_bwd_reference_host.py).

Out of scope, the next slice: the float32 engine's backward chain (tr_backward has none of the epilogue fusions; its step is held to 1e-5
against float64 autograd by tests/test_gpu_train.py).

FOUND AND FIXED (test_tapped_backward_is_bit_identical_to_the_untapped_step[resnet50-29-96] is the regression test; it failed in most runs
before the fix).  With the side stream on (the default) the STEM's gradients of a plain dh_train2_backward were not reproducible from run to
run at ResNet-50 P = 96 from about B = 28: of 39 identical untapped steps at B = 32, 8 to 39 differed from the first in conv1.weight,
bn1.weight and bn1.bias -- and in nothing else of the arena -- in one to six whole channels, by up to 3 % of the largest dgamma, and the
stem's dZ in the same channels (0 of 39 at B = 16, 0 of 29 at B = 32 with DH_T2_SIDE=0; fewer side-stream workgroups made it rarer: 4 of
39 with DH_WGRAD_RING_WGS=16 DH_WGRAD2_WGS=16; the LDS-DMA ring kernel is not needed for it: 8 of 39 with DH_WGRAD_RING=0).  Between such
runs Z, X1, the pooled gradient the stem read (this module's tap), mean, invstd and the dZ of layer 1 are bit-identical: the column sums of
bn2_pool_bwd_reduce_kernel changed while the side stream's weight gradients of layer 1 ran beside it, each time by about one routed
pool-gradient element (ddgamma / ddbeta between 1 and 2.5: a strongly positive xhat, a pool winner).  The affected channels were those of
particular vector elements (c mod 4 == 2) and moved to other elements when the byte test of pool_grad_2x2 was written differently, so the
fault sits in that kernel's execution beside other work, not in a shared buffer; which instruction is at fault is NOT known.  The fix is in
the host code: t2_backward joins the side stream IN FRONT of the stem's tail instead of behind it (nothing is handed to the side stream
after that point), so the tail runs alone as it does with DH_T2_SIDE=0: 0 of 158 steps differ at B = 32 (default and DH_T2_FOLD=0).

Measured on an MI355X (records only, no threshold is derived from them; all 23 tests pass, the file takes 11.3 s wall, the slowest
test -- B = 29 with its 106 tapped steps -- 4.3 s), in the order of the cases:
  lowest identical fraction of dZ        1.0000 | 0.9999 layer3.2.conv1 | 0.9999 layer1.1.conv2 | 0.9999 layer1.0.conv1 | 0.9999 layer3.4.conv2
                                         (stem: 0.9999 | 0.9999 | 1.0000 | 1.0000 | 0.9998)
  lowest identical fraction of grad_in   0.9998 layer2.0.conv2 | 0.9994 layer4.0.conv2 | 0.9997 layer3.0.conv2 | 0.9997 layer4.1.conv1 |
                                         0.9997 layer4.2.conv1
  largest |got - want| / gate of dZ      0.9999 in every case (layer2.0.conv1 | layer1.2.conv3 | layer2.2.conv2 | layer1.1.conv2 | layer1.1.conv2):
                                         an element one bf16 unit from `want`, which is the gate's first term
  ... of grad_in                         0.968 conv1 (the pooled gradient) | 0.997 layer1.1.conv3 | 0.999 layer1.0.conv3 | 0.9999 | 0.9999 (the
                                         head's gradient of the last block in the last two)
  largest channel sum / any-order bound  dgamma or dbeta: 0.055 layer4.0.conv1 | 0.104 layer4.0.downsample.0 | 0.121 layer4.2.conv3 |
                                         0.041 layer4.1.conv2 | 0.0055 layer4.1.conv3 (stem: 9e-6 | 2e-5 | 2e-5 | 7e-6 | 8e-7)
  largest relative L2 of dgamma / dbeta  2.3e-7 / 3.0e-8 | 2.5e-7 / 2.0e-8 | 2.1e-7 / 2.6e-8 | 2.0e-7 / 2.8e-8 | 3.6e-7 / 3.9e-8 (gate 1e-5)
  undecided ReLU share (cap 1e-4)        2.2e-5 layer3.1.conv1 | 0 | 0 | 0 | 3.7e-6;  undecided pool windows (cap 1e-2): 0.0076 | 0.0075 |
                                         0.0048 | 0.0049 | 0.0083
  routes                                 all sixteen reached (test_every_route_of_t2_backward_is_reached prints the list)
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import layer_ref as lr
from oracle import resnet18 as o18
from oracle import resnet50 as o50
from oracle import step_bwd_ref as sb

pytestmark = pytest.mark.gpu

CASES = [c[:3] for c in sb.STEP_CASES]
DRAW = {c[:3]: c[3] for c in sb.STEP_CASES}
SEED, IMAGES = sb.STEP_SEED, sb.STEP_IMAGES


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(arch, dev):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    ref = (o50 if arch == "resnet50" else o18).seeded_model(SEED[arch], 5, perturb_bn=True)
    m = get_model(5, "bf16", arch=arch)
    m.load_state_dict(ref.state_dict())
    return ref, m.to(dev).train()


def _shapes(ref, B, P):
    """[B][C][H][W] of every conv output and of the pooled stem map."""
    shapes = {}
    hooks = [mod.register_forward_hook(lambda _m, _i, out, n=n: shapes.__setitem__(n, (B,) + tuple(out.shape[1:])))
             for n, mod in ref.named_modules() if isinstance(mod, torch.nn.Conv2d)]
    with torch.no_grad():
        ref.eval()(torch.zeros(1, 3, P, P))
    for h in hooks:
        h.remove()
    h2 = (shapes["conv1"][2] - 1) // 2 + 1
    shapes["maxpool"] = (B, 64, h2, h2)
    return shapes


def _nchw(buf, shape):
    b, c, h, w = shape
    return np.ascontiguousarray(buf.cpu().numpy().reshape(b, h, w, c).transpose(0, 3, 1, 2))


def _act(eng, name, what, shape, dev):
    from deephisto_amd._lib import check, lib
    buf = torch.empty(int(np.prod(shape)), dtype=torch.float32, device=dev)
    check(lib().dh_train2_debug_act(eng.handle, name.encode(), what, buf.data_ptr(), buf.numel(), None), f"debug_act {name} what={what}")
    return _nchw(buf, shape)


def _tap_call(eng, dl, name, n, want_g_out, dev, cout):
    """One tapped backward: (rc, grad_in, g_out, mean, invstd, route) with the tensors still on the device."""
    from deephisto_amd._lib import lib
    gin = torch.empty(n, dtype=torch.float32, device=dev)
    gout = torch.empty(n, dtype=torch.float32, device=dev) if want_g_out else None
    mean, invstd = torch.empty(cout, dtype=torch.float32, device=dev), torch.empty(cout, dtype=torch.float32, device=dev)
    route = (C.c_int32 * sb.ROUTE_N)(*([-7] * sb.ROUTE_N))
    rc = lib().dh_train2_debug_backward_tap(eng.handle, dl.data_ptr(), name.encode(), gin.data_ptr(), n, gout.data_ptr() if want_g_out else None,
                                            mean.data_ptr(), invstd.data_ptr(), route, None)
    return rc, gin, gout, mean, invstd, list(route)


@functools.lru_cache(maxsize=None)
def _step(case):
    """One case: an untapped step, then one forward + tapped backward per BN; the step as oracle.step_bwd_ref reads it, and what (d) compares."""
    arch, B, P = case
    dev = torch.device("cuda:0")
    ref, m = _model(arch, dev)
    eng = m._engine
    topo = lr.topology(ref)
    shapes = _shapes(ref, B, P)
    x, labels = (t.to(dev) for t in sb.case_inputs(B, P, DRAW[case]))
    sd = ref.state_dict()
    s = dict(topo=topo, B=B, images=IMAGES.get(B), Z={}, Y={}, dz={}, tap={}, w={}, gamma={}, beta={}, dgamma={}, dbeta={})
    for L in topo:
        s["w"][L["name"]] = sd[L["name"] + ".weight"].bfloat16().double().numpy()
        s["gamma"][L["bn"]], s["beta"][L["bn"]] = sd[L["bn"] + ".weight"].numpy(), sd[L["bn"] + ".bias"].numpy()
    s["fc_w"] = sd["fc.weight"].numpy()
    # the untapped step
    m.zero_grad(set_to_none=True)
    F.cross_entropy(m(x), labels).backward()
    torch.cuda.synchronize()
    for L in topo:
        s["dgamma"][L["bn"]] = dict(m.named_parameters())[L["bn"] + ".weight"].grad.cpu().numpy().copy()
        s["dbeta"][L["bn"]] = dict(m.named_parameters())[L["bn"] + ".bias"].grad.cpu().numpy().copy()
    arena1 = eng.flat(1, dev).clone()
    dz1 = {L["name"]: _act(eng, L["name"], 2, shapes[L["name"]], dev) for L in topo}
    # one forward and one tapped backward per BN
    blks = sb.blocks(topo)
    writes = {b["top"] for bi, b in enumerate(blks) if not sb.premasked(s, blks, bi)}
    same = dict(arena=[], dz=[], twice=[])
    for L in topo:
        name = L["name"]
        shape = shapes["maxpool"] if name == "conv1" else shapes[name]
        with torch.no_grad():
            logits = m(x)
        if "dlogits" not in s:
            lg = logits.detach().clone().requires_grad_(True)
            F.cross_entropy(lg, labels).backward()
            dl = lg.grad.contiguous()
            s["dlogits"] = dl.cpu().numpy()
        rc, gin, gout, mean, invstd, route = _tap_call(eng, dl, name, int(np.prod(shape)), name in writes, dev, shapes[name][1])
        assert rc == 0, (name, rc)
        same["arena"].append((name, bool(torch.equal(eng.flat(1, dev).view(torch.int32), arena1.view(torch.int32)))))
        dz = _act(eng, name, 2, shapes[name], dev)
        same["dz"].append((name, bool(np.array_equal(dz.view(np.uint32), dz1[name].view(np.uint32)))))
        if B > 16:      # images outside the float64 selection: two tapped runs, bit for bit
            with torch.no_grad():
                m(x)
            rc, gin2, gout2, *_ = _tap_call(eng, dl, name, int(np.prod(shape)), name in writes, dev, shapes[name][1])
            assert rc == 0, (name, rc)
            same["twice"].append((name, bool(torch.equal(gin.view(torch.int32), gin2.view(torch.int32))) and
                                  (gout is None or bool(torch.equal(gout.view(torch.int32), gout2.view(torch.int32))))))
        s["tap"][name] = dict(grad_in=_nchw(gin, shape), g_out=None if gout is None else _nchw(gout, shape), mean=mean.cpu().numpy(),
                              invstd=invstd.cpu().numpy(), route=route)
    # what the last forward / backward left: identical every time (same parameters, same input)
    dz2 = {L["name"]: _act(eng, L["name"], 2, shapes[L["name"]], dev) for L in topo}
    same["dz_all"] = [(n, bool(np.array_equal(d.view(np.uint32), dz1[n].view(np.uint32)))) for n, d in dz2.items()]
    s["dz"] = dz1
    s["Z"] = {L["name"]: _act(eng, L["name"], 0, shapes[L["name"]], dev) for L in topo}
    s["Y"] = {L["name"]: _act(eng, L["name"], 1, shapes[L["name"]], dev) for L in topo[1:] if ".downsample" not in L["name"]}
    s["same"] = same
    torch.cuda.synchronize()
    m._release()
    return s


def _assert_clean(case, reps):
    fig = sb.figures(reps)
    print(f"\n[step bwd] {case}: " + ", ".join(f"{k} {v[0]:.4g} ({v[1]})" for k, v in fig.items()))
    bad = [f for r in reps for f in r.failures]
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("arch,B,P", CASES)
def test_every_bn_backward_matches_float64(dev, arch, B, P):
    s = _step((arch, B, P))
    _assert_clean((arch, B, P), [sb.judge_bn(s, L) for L in s["topo"][1:]])


@pytest.mark.parametrize("arch,B,P", CASES)
def test_every_incoming_gradient_matches_the_float64_dgrad_of_its_producer(dev, arch, B, P):
    s = _step((arch, B, P))
    reps = sb.judge_chain(s)
    n_ds = sum(".downsample" in L["name"] for L in s["topo"])     # a downsample BN reads its block's identity gradient: held to equality with it
    assert len([r for r in reps if "grad_in" in r.name]) == len(s["topo"]) - n_ds      # every other grad_in is some dgrad's (or the head's) output
    _assert_clean((arch, B, P), reps)


@pytest.mark.parametrize("arch,B,P", CASES)
def test_stem_tail_matches_the_pool_reference(dev, arch, B, P):
    _assert_clean((arch, B, P), [sb.judge_stem(_step((arch, B, P)))])


@pytest.mark.parametrize("arch,B,P", CASES)
def test_tapped_backward_is_bit_identical_to_the_untapped_step(dev, arch, B, P):
    same = _step((arch, B, P))["same"]
    for key in ("arena", "dz", "dz_all", "twice"):
        assert len(same[key]) >= 20 or (key == "twice" and B <= 16), key
        assert all(ok for _, ok in same[key]), (key, [n for n, ok in same[key] if not ok])


def test_every_route_of_t2_backward_is_reached(dev):
    routes = []
    for case in CASES:
        s = _step(case)
        ks = {L["name"]: s["w"][L["name"]].shape[-1] for L in s["topo"]}
        routes += [(case, n, ks[n], t["route"]) for n, t in s["tap"].items()]
    R = sb
    reached = {
        "ReLU mode 0": any(r[R.R_RELU] == 0 for *_, r in routes),
        "ReLU mode 1": any(r[R.R_RELU] == 1 for *_, r in routes),
        "ReLU mode 2": any(r[R.R_RELU] == 2 for *_, r in routes),
        "pre-masked": any(r[R.R_PREMASKED] == 1 for *_, r in routes),
        "not pre-masked": any(r[R.R_PREMASKED] == 0 for *_, r in routes),
        "in_mask used": any(r[R.R_IN_MASK] == 1 for *_, r in routes),
        "in_mask not used": any(r[R.R_IN_MASK] == 0 for *_, r in routes),
        "epilogue sums for a 3x3 conv's BN": any(r[R.R_HAVE_ROWS] > 0 and k == 3 and r[R.R_RELU] == 2 for _, _, k, r in routes),
        "epilogue sums for a pre-masked join BN (top_rows)": any(r[R.R_HAVE_ROWS] > 0 and r[R.R_PREMASKED] == 1 and r[R.R_RELU] == 0 for *_, r in routes),
        "own reduction, channel-sliced": any(r[R.R_REDUCE] == R.REDUCE_SLICED for *_, r in routes),
        "own reduction, bn2_bwd_reduce_kernel": any(r[R.R_REDUCE] == R.REDUCE_BLOCKS for *_, r in routes),
        "fold": any(r[R.R_APPLY] == R.APPLY_FOLD for *_, r in routes),
        "finalize + apply": any(r[R.R_APPLY] == R.APPLY_FINALIZE and r[R.R_REDUCE] != R.REDUCE_POOL for *_, r in routes),
        "finalize + apply on epilogue sums": any(r[R.R_APPLY] == R.APPLY_FINALIZE and r[R.R_HAVE_ROWS] > 0 for *_, r in routes),
        "a downsample block": any(r[R.R_BRANCH] == 2 for *_, r in routes) and any(r[R.R_BRANCH] == 1 for *_, r in routes),
        "the stem's pool reduction": any(r[R.R_REDUCE] == R.REDUCE_POOL for *_, r in routes),
    }
    print("\n[step bwd] routes reached: " + ", ".join(f"{k}: {'yes' if v else 'NO'}" for k, v in reached.items()))
    assert all(reached.values()), [k for k, v in reached.items() if not v]
    assert all(all(v >= 0 for v in r) for *_, r in routes)      # every field of every record was written


@pytest.mark.parametrize("arch", ["resnet18", "resnet50"])
def test_refusals_name_the_argument(dev, arch):
    from deephisto_amd._lib import lib
    B, P = 2, 64
    ref, m = _model(arch, dev)
    eng = m._engine
    shapes = _shapes(ref, B, P)
    topo = lr.topology(ref)
    x = torch.rand(B, 3, P, P).to(dev)
    dl = (torch.randn(B, 5) / B).to(dev)
    inner, top_last = "layer1.0.conv1", topo[-1]["name"]
    n = lambda name: int(np.prod(shapes["maxpool"] if name == "conv1" else shapes[name]))  # noqa: E731

    def refused(name, n_elem, g_out, *words, null=None):
        rc, *_ = _tap_call(eng, dl, name, n_elem, g_out, dev, 2048) if null is None else (null(),)
        assert rc == -22, (name, n_elem, g_out, rc)
        err = lib().dh_last_error()
        assert all(w in err for w in words), err

    with torch.no_grad():
        m(x)
    refused("layer9.0.conv1", n(inner), False, b"conv_name")
    refused(inner, n(inner) - 8, False, b"n_elem")
    refused("conv1", int(np.prod(shapes["conv1"])), False, b"n_elem")        # the stem's grad_in is the POOLED gradient
    refused(inner, n(inner), True, b"g_out_dev")                              # an inner BN writes no masked gradient
    refused("conv1", n("conv1"), True, b"g_out_dev")
    refused("layer2.0.downsample.0", n("layer2.0.downsample.0"), True, b"g_out_dev")
    if arch == "resnet50":                                                    # layer1.0's successor starts with a stride-1 1x1 conv: pre-masked
        refused("layer1.0.conv3", n("layer1.0.conv3"), True, b"g_out_dev")
    buf = torch.empty(n(inner), dtype=torch.float32, device=dev)
    refused(inner, 0, False, b"null", null=lambda: lib().dh_train2_debug_backward_tap(
        eng.handle, dl.data_ptr(), inner.encode(), buf.data_ptr(), buf.numel(), None, buf.data_ptr(), buf.data_ptr(), None, None))
    # none of the refusals consumed the forward: a tapped backward still runs, with g_out where one is written, and NULL is accepted there too
    rc, *_, route = _tap_call(eng, dl, top_last, n(top_last), True, dev, shapes[top_last][1])
    assert rc == 0 and route[sb.R_RELU] == 1 and route[sb.R_PREMASKED] == 0
    refused(inner, n(inner), False, b"forward")                               # no forward since that backward
    with torch.no_grad():
        m(x)
    rc, *_ = _tap_call(eng, dl, top_last, n(top_last), False, dev, shapes[top_last][1])
    assert rc == 0
    with torch.no_grad():
        m(x)
    assert lib().dh_train2_backward(eng.handle, dl.data_ptr(), None) == 0     # an untapped backward ...
    refused(inner, n(inner), False, b"forward")                               # ... ends the step as well
    torch.cuda.synchronize()
    m._release()
