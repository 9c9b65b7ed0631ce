"""Launched by tests/test_gpu_train_vs_parent.py in a fresh process per (library, side-stream switch): training steps of the three engines
(ResNet-18 float32, ResNet-18 bf16, ResNet-50 bf16) through the PRODUCT entry points only, so the parent commit's library loads under the same
bindings; saves every result to argv[1] (.npz, raw bits).  argv[2], optional: another build of the library to load instead of the in-tree one --
the parent commit's (tools/vs_parent.sh).  DH_T1_SIDE / DH_T2_SIDE come from the caller's environment.

Every run starts from seeded_model(seed, 5, perturb_bn=True) on x = rand(4, 3, 64, 64): the smallest patch either engine accepts; it reaches every
block shape, both downsample kinds and the 1x1 per-tap weight gradient.
  fused    three fused train_steps (backward_adam: the optimiser and the repack ride the side stream behind each group's weight gradients)
  unfused  three train_steps with fuse_optimizer = False (backward, then adam_step)
  bucket   one forward, one backward with a recording bucket callback at 1 MiB (the joins in front of every due bucket): the flat gradient
           arena and the fired (bucket, offset, count) list, then adam_step
  shape    fused steps at B = 4, 2, 4 (the batch-shape change re-makes the activations and keeps the optimiser state)
Saved per run: every step's loss and logits, the gradient arena of `bucket`, the final state_dict."""
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(REPO))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from deephisto_amd import _lib  # noqa: E402

if __name__ == "__main__" and len(sys.argv) > 2:
    _lib.LIB_PATH = Path(sys.argv[2]).resolve()

ENGINES = [("r18_f32", "resnet18", "f32"), ("r18_bf16", "resnet18", "bf16"), ("r50_bf16", "resnet50", "bf16")]
N_STATE = {"resnet18": 122, "resnet50": 320}   # state_dict entries: convs + 5 per BN + fc weight and bias
RUN_ARRAYS = {"fused": 6, "unfused": 6, "bucket": 3, "shape": 6}   # besides the state_dict
MIN_ARRAYS = sum(sum(RUN_ARRAYS.values()) + len(RUN_ARRAYS) * N_STATE[arch] for _, arch, _ in ENGINES)
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8
BUCKET_BYTES = 1024 * 1024


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.numpy().view(np.int32) if t.dtype == torch.float32 else t.numpy()


def _model(dev, arch, dtype, seed):
    from deephisto_amd.models.patch_cls_simple.model import get_model
    from oracle import resnet18 as o18
    from oracle import resnet50 as o50
    m = get_model(5, dtype) if dtype == "f32" else get_model(5, dtype, arch=arch)
    m.load_state_dict((o50 if arch == "resnet50" else o18).seeded_model(seed, 5, perturb_bn=True).state_dict())
    return m.to(dev).train()


def _save_state(m, arch, key, saved):
    sd = m.state_dict()
    assert len(sd) == N_STATE[arch], (arch, len(sd))
    for name, t in sd.items():
        saved[f"{key}_sd_{name}"] = _bits(t)


def _steps(m, x, y, batches, key, saved):
    for i, B in enumerate(batches):
        loss, logits = m.train_step(x[:B], y[:B], lr=LR, betas=BETAS, eps=EPS)
        saved[f"{key}_loss{i}"] = _bits(loss.reshape(1))
        saved[f"{key}_logits{i}"] = _bits(logits)


def _bucket_run(m, x, y, key, saved):
    from deephisto_amd._lib import BUCKET_CB
    from deephisto_amd.models.patch_cls_simple.engine import _stream, ce_loss
    eng = m._engine if hasattr(m, "_engine") else m._engine2
    st = _stream(x.device)
    logits = eng.forward(x, True, pull_stats=False)
    _, dl = ce_loss(logits, y, want_grad=True)
    fired = []
    cb = BUCKET_CB(lambda b, off, cnt, _u: fired.append((b, off, cnt)))
    eng._call("set_buckets", BUCKET_BYTES, cb, None, None)
    try:
        eng._call("backward", dl.data_ptr(), st)
    finally:
        eng._call("set_buckets", 0, None, None, None)
    torch.cuda.synchronize()
    assert len(fired) > 1, fired
    saved[f"{key}_logits"] = _bits(logits)
    saved[f"{key}_grads"] = _bits(eng.flat(1, x.device).clone())
    saved[f"{key}_fired"] = np.asarray(fired, dtype=np.int64)
    eng._call("adam_step", LR, BETAS[0], BETAS[1], EPS, 0, st)
    eng.native_ahead = True


def main():
    dev = torch.device("cuda:0")
    saved = {}
    for tag, arch, dtype in ENGINES:
        seed = 7 + len(tag) + len(arch)
        g = torch.Generator().manual_seed(seed)
        x = torch.rand(4, 3, 64, 64, generator=g).to(dev)
        y = torch.randint(0, 5, (4,), generator=g).to(dev)
        for run in RUN_ARRAYS:
            m = _model(dev, arch, dtype, seed)
            key = f"{tag}_{run}"
            before = len(saved)
            if run == "bucket":
                _bucket_run(m, x, y, key, saved)
            else:
                m.fuse_optimizer = run != "unfused"
                _steps(m, x, y, (4, 2, 4) if run == "shape" else (4, 4, 4), key, saved)
            assert len(saved) - before == RUN_ARRAYS[run], (key, len(saved) - before)
            _save_state(m, arch, key, saved)
            del m
    assert len(saved) == MIN_ARRAYS, (len(saved), MIN_ARRAYS)
    np.savez(sys.argv[1], **saved)


if __name__ == "__main__":
    main()
