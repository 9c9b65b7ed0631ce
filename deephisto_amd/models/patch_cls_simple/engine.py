"""The native-engine layer both patch classifiers share (`ResNet18HIP` in model.py, `ResNet50HIP` in resnet_bf16.py).

`ResNetHIP` is an `nn.Module` with torchvision's ResNet `state_dict` layout (so `best_model.pth` files interchange,
examples/predict_full_patched.py:116-126) whose sub-modules are parameter *holders* only: libdeephisto_hip.so computes.
Two kinds of native handle serve it:
- inference handles (`<ABI>_set_param`, `_finalize`, `_forward`, `_forward_tiles`, `_destroy`), one per lane, each with its own
  activation workspace, re-synced from the `state_dict` whenever a parameter or running statistic moved;
- a training engine (`_Trainer`, the model's `_engine`): f32 master weights, gradients, Adam moments and running statistics in HBM
  behind seven entry points both engines share (`_ENTRIES`: tensor, flat, set_buckets, bucket, backward, backward_adam, adam_step;
  one table per engine names their symbols).  `_F32Trainer` (ResNet-18 in float32, `dh_resnet18_train_*`) keeps its state inside
  the model's lane-0 inference handle; `_Train2Trainer` (ResNet-50, and ResNet-18 in bf16: `dh_train2_*`) owns a handle of its own.
The step they replace is models/patch_cls_simple/train.py:166-172 (`outputs = model(inputs)`, `criterion`, `loss.backward()`,
`optimizer.step()`).  Data-parallel training (one process per GPU, RCCL): the gradient arena is laid out in backward-completion order
and cut into ~25 MB buckets; each bucket's all-reduce starts on a side stream as soon as the backward kernels that complete it are
enqueued, Adam waits for the last one.
"""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from ..._lib import BUCKET_CB, check, lib
from ...tiles import _stream
from .ddp import DEFAULT_BUCKET_BYTES, BucketReducer


class _DevView:
    """float32 device memory owned by the native library, exposed through the CUDA array interface."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<f4", "data": (ptr, False), "version": 2}


def ce_loss(logits: torch.Tensor, labels: torch.Tensor, want_grad: bool = False):
    """Mean cross entropy of float32[n, n_cls] logits against int64 labels on the GPU (`dh_ce_loss`:
    nn.CrossEntropyLoss() of train.py:117).  Returns the scalar loss tensor, or (loss, dlogits) with
    dlogits = (softmax - onehot) / n when `want_grad`."""
    if not logits.is_cuda:
        raise RuntimeError("ce_loss runs on the GPU only")
    logits = logits.detach().to(torch.float32).contiguous()
    labels = labels.to(device=logits.device, dtype=torch.int64).contiguous()
    loss = torch.empty((), dtype=torch.float32, device=logits.device)
    dl = torch.empty_like(logits) if want_grad else None
    check(lib().dh_ce_loss(logits.data_ptr(), labels.data_ptr(), logits.shape[0], logits.shape[1], loss.data_ptr(),
                           dl.data_ptr() if want_grad else None, _stream(logits.device)), "dh_ce_loss")
    return (loss, dl) if want_grad else loss


_ENTRIES = ("tensor", "flat", "set_buckets", "bucket", "backward", "backward_adam", "adam_step")


class _Trainer:
    """Training state of `module` in the library, kept consistent with the module's tensors: parameters and running statistics
    changed on the torch side (optimizer step, load_state_dict) are pushed before the next training forward, found by
    (data_ptr, version counter); what fused `train_step` calls left newer in the library is pulled back on demand.  Subclasses open
    the handle and run the raw forward (`_forward`)."""

    ENTRY: dict = {}   # role in _ENTRIES -> the engine's C symbol

    def __init__(self, module: nn.Module):
        self.module, self.n_classes = module, module.n_classes
        self.handle = None
        self._pushed = {}           # tensor name -> (data_ptr, version) last copied into the library
        self._stats_pending = 0     # training forwards whose running statistics were not pulled yet
        self.native_ahead = False   # the library's parameters are newer than the nn.Parameters (fused train_step)
        self.generation = 0         # bumped by every training forward: the library's parameters / running statistics may have moved
        self._cb = None
        self.overlap_log = []       # (bucket, offset, count) in launch order of the last data-parallel backward (tests, bench.py)
        self.ddp_wire = None        # gradient wire format of data-parallel steps: None = DH_DDP_WIRE (default f32), "f32", "bf16"
        self.fuse_optimizer = True  # single-rank train_step: backward_adam (False: backward, then adam_step; tests)

    def _call(self, entry: str, *args, what: str | None = None):
        name = self.ENTRY[entry]
        check(getattr(lib(), name)(self.handle, *args), what or name)

    def _tensors(self):
        """(kind, name, tensor) of what the library holds: parameters (kind 0) and running statistics (kind 2)."""
        for kind, items in ((0, self.module.named_parameters()), (2, self.module.named_buffers())):
            for name, t in items:
                if not name.endswith("num_batches_tracked"):
                    yield kind, name, t

    def _mark_pushed(self, name, t):
        self._pushed[name] = (t.data_ptr(), t._version)

    def release(self):
        self.handle = None

    # ---- parameter traffic ------------------------------------------------------------------------------
    def push_changed(self, dev) -> bool:
        """nn.Parameters / buffers changed since the last push -> library.  True when a parameter was pushed."""
        if self.native_ahead:
            return False
        st, params = _stream(dev), False
        for kind, name, t in self._tensors():
            if self._pushed.get(name) != (t.data_ptr(), t._version):
                src = t.detach().to(device=dev, dtype=torch.float32).contiguous()
                self._call("tensor", name.encode(), kind, src.data_ptr(), src.numel(), 1, st, what=f"push {name}")
                self._mark_pushed(name, t)
                params |= kind == 0
        return params

    def pull_running_stats(self):
        """Library running statistics -> module buffers (+ the batch counters owed since the last pull)."""
        if not self._stats_pending or self.handle is None:
            return
        with torch.no_grad():
            for name, buf in self.module.named_buffers():
                if name.endswith("num_batches_tracked"):
                    buf += self._stats_pending
                else:
                    self._call("tensor", name.encode(), 2, buf.data_ptr(), buf.numel(), 0, _stream(buf.device), what=f"pull {name}")
                    self._mark_pushed(name, buf)
        self._stats_pending = 0

    def pull_parameters(self):
        """Library masters and running statistics -> nn.Parameters / buffers (after fused train_step calls)."""
        self.pull_running_stats()
        if self.native_ahead and self.handle is not None:
            with torch.no_grad():
                for name, prm in self.module.named_parameters():
                    self._call("tensor", name.encode(), 0, prm.data_ptr(), prm.numel(), 0, _stream(prm.device), what=f"pull {name}")
                    self._mark_pushed(name, prm)
            self.native_ahead = False

    # ---- forward / backward -----------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, training: bool = True, pull_stats: bool = True) -> torch.Tensor:
        """float32[n, 3, P, P] on the GPU -> float32[n, n_classes] logits.  `training`: batch-statistic BN, running statistics
        updated, x must stay alive until backward."""
        out = torch.empty((int(x.shape[0]), self.n_classes), dtype=torch.float32, device=x.device)
        self._forward(x, out, training, _stream(x.device))
        if training:
            self.generation += 1
            self._stats_pending += 1
            if pull_stats:
                self.pull_running_stats()
        return out

    def backward(self, dlogits: torch.Tensor):
        """dlogits float32[n, n_classes] -> the gradient of every parameter (None where it does not require one)."""
        st = _stream(dlogits.device)
        self._call("backward", dlogits.data_ptr(), st)
        grads = []
        for name, prm in self.module.named_parameters():
            g = torch.empty_like(prm, dtype=torch.float32)
            self._call("tensor", name.encode(), 1, g.data_ptr(), g.numel(), 0, st, what=f"grad {name}")
            grads.append(g if prm.requires_grad else None)
        return grads

    def flat(self, kind: int, dev) -> torch.Tensor:
        """A whole arena (kind 0 parameters, 1 gradients, 2 running statistics) as one float32 tensor view (no copy)."""
        ptr, n = C.c_void_p(), C.c_int64()
        self._call("flat", kind, C.byref(ptr), C.byref(n))
        return torch.as_tensor(_DevView(ptr.value, n.value), device=dev)

    # ---- data-parallel gradient exchange ------------------------------------------------------------------
    def bucket_ranges(self, bucket_bytes: int = DEFAULT_BUCKET_BYTES):
        """[(offset, count)] of the gradient buckets in completion order (fc first, stem last)."""
        n = C.c_int32()
        self._call("set_buckets", int(bucket_bytes), None, None, C.byref(n))
        out = []
        for i in range(n.value):
            off, cnt = C.c_int64(), C.c_int64()
            self._call("bucket", i, C.byref(off), C.byref(cnt))
            out.append((off.value, cnt.value))
        return out

    def _arm_overlap(self, dev, group, bucket_bytes):
        red = BucketReducer(self.flat(1, dev), group, self.ddp_wire)
        # called inside backward right after the kernels completing a bucket were enqueued on the current stream
        self._cb = BUCKET_CB(lambda bucket, off, cnt, _user: red.on_bucket(bucket, off, cnt))   # keep the trampoline alive
        self._call("set_buckets", int(bucket_bytes), self._cb, None, None)
        return red

    def _finish_overlap(self, red, ok=True):
        try:
            if ok:
                red.finish()
                self.overlap_log = red.log
        finally:   # never leave the library holding a callback into a dead trampoline
            self._call("set_buckets", 0, None, None, None)
            self._cb = None

    def train_step(self, x, labels, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, group=None, bucket_bytes=DEFAULT_BUCKET_BYTES):
        """Fused step in HIP: forward (batch-statistic BN), CrossEntropy(mean), backward, [bucketed all-reduce overlapped with the
        backward kernels], Adam.  Adam passes step 0: the library counts the steps of its moments."""
        import torch.distributed as dist

        x = x.detach().to(torch.float32).contiguous()
        logits = self.forward(x, pull_stats=False)   # 40 small copies per step otherwise; pulled lazily
        loss, dl = ce_loss(logits, labels, want_grad=True)
        st = _stream(x.device)
        world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        if world == 1 and self.fuse_optimizer:   # no gradient exchange: the update rides behind each block's weight gradients
            self._call("backward_adam", dl.data_ptr(), lr, betas[0], betas[1], eps, 0, st)
            self.native_ahead = True
            return loss, logits
        red = self._arm_overlap(x.device, group, bucket_bytes) if world > 1 else None
        try:
            self._call("backward", dl.data_ptr(), st)
        except Exception:
            if red is not None:
                self._finish_overlap(red, ok=False)
            raise
        if red is not None:
            self._finish_overlap(red)
        self._call("adam_step", lr, betas[0], betas[1], eps, 0, st)
        self.native_ahead = True
        return loss, logits


class _F32Trainer(_Trainer):
    """ResNet-18 in float32 (`dh_resnet18_train_*`).  The library keeps this training state inside an inference handle: the trainer
    borrows the model's lane 0, and the first `train_begin` copies that handle's parameters into fresh masters."""

    ENTRY = {e: f"dh_resnet18_{e}" for e in _ENTRIES} | {"tensor": "dh_resnet18_train_tensor", "flat": "dh_resnet18_train_flat"}

    def _forward(self, x, out, training, st):
        if not training:
            raise ValueError("the float32 training engine has no eval forward: eval() runs the inference handle")
        n, p = int(x.shape[0]), int(x.shape[2])
        if self.handle is None:
            self.handle = self.module.lane_handles(1)[0]
            for _, name, t in self._tensors():   # what train_begin is about to copy in
                self._mark_pushed(name, t)
        check(lib().dh_resnet18_train_begin(self.handle, n, p, st), "dh_resnet18_train_begin")
        if self.push_changed(x.device):
            check(lib().dh_resnet18_train_repack(self.handle, st), "dh_resnet18_train_repack")
        check(lib().dh_resnet18_forward_train(self.handle, x.data_ptr(), n, p, out.data_ptr(), st), "dh_resnet18_forward_train")


class _Train2Trainer(_Trainer):
    """The bf16 engine (`dh_train2_*`: bf16 activations and MFMA with f32 accumulation for forward, dgrad and wgrad; f32 masters,
    gradients and Adam) on a handle of its own."""

    ENTRY = {e: f"dh_train2_{e}" for e in _ENTRIES}

    def __init__(self, module: nn.Module, arch: str):
        super().__init__(module)
        self.arch = arch

    def _forward(self, x, out, training, st):
        if self.handle is None:
            h = C.c_void_p()
            check(lib().dh_train2_create(C.byref(h), self.arch.encode(), self.n_classes), "dh_train2_create")
            self.handle = h
        self.push_changed(x.device)
        check(lib().dh_train2_forward(self.handle, x.data_ptr(), int(x.shape[0]), int(x.shape[2]), out.data_ptr(),
                                      1 if training else 0, st), "dh_train2_forward")

    def release(self):
        if self.handle is not None:
            lib().dh_train2_destroy(self.handle)
        self.handle = None


class _TrainForward(torch.autograd.Function):
    """logits = model(x) in training mode; backward runs the HIP backward kernels and hands every parameter its gradient (so
    `loss.backward(); optimizer.step()` of models/patch_cls_simple/train.py:171-172 work unchanged on the nn.Parameters)."""

    @staticmethod
    def forward(ctx, x, trainer, *params):
        trainer.pull_parameters()   # a torch optimizer will step the nn.Parameters: they must hold the library's newest values
        ctx.trainer, ctx.x = trainer, x   # x must outlive backward (the stem wgrad reads it)
        return trainer.forward(x)

    @staticmethod
    def backward(ctx, dlogits):
        return (None, None, *ctx.trainer.backward(dlogits.to(torch.float32).contiguous()))


class ResNetHIP(nn.Module):
    """A ResNet patch classifier on the native engines.  Subclasses give the residual blocks (`stages`: an iterable of block lists,
    built as it is consumed so that the parameters are initialised in torchvision's order), the inference ABI (`ABI`,
    `_create_handle`), the trainer (`_new_trainer`) and the eval forward (`_forward_eval`)."""

    ABI = ""   # prefix of the inference entry points

    def __init__(self, n_classes: int, compute_dtype: str, stages, width: int):
        super().__init__()
        self.n_classes = int(n_classes)
        self.compute_dtype = compute_dtype
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        for i, blocks in enumerate(stages, start=1):
            setattr(self, f"layer{i}", nn.Sequential(*blocks))
        self.fc = nn.Linear(width, n_classes)
        for m in self.modules():  # torchvision's ResNet initialisation
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm2d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        self._lanes = []   # inference handles: [handle, signature of the parameters it holds]
        self._engine = self._new_trainer()   # touches the library only on its first training forward

    def _release(self):
        self._engine.release()
        for lane in self._lanes:
            if lane[0]:
                getattr(lib(), f"{self.ABI}_destroy")(lane[0])
        self._lanes = []

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    # ---- inference handles -----------------------------------------------------------------------------
    def lane_handles(self, n: int):
        """n inference handles holding the current parameters (re-synced whenever parameters or running statistics changed), each
        with its own activation workspace, so that n launches can be in flight on n HIP streams."""
        n = max(1, n)
        # state_dict() first pulls what fused train_step calls left in the library; `generation` covers the running statistics
        # training forwards wrote in place (no version bump)
        sd = self.state_dict(keep_vars=True)
        sig = (self._engine.generation,) + tuple((k, v.data_ptr(), v._version) for k, v in sd.items())
        while len(self._lanes) < n:
            self._lanes.append([C.c_void_p(), None])
        stale = [lane for lane in self._lanes[:n] if lane[1] != sig]
        host = [(k, v.detach().to("cpu", torch.float32).contiguous()) for k, v in sd.items()
                if not k.endswith("num_batches_tracked")] if stale else []
        for lane in stale:
            if not lane[0]:
                check(self._create_handle(lane[0]), f"{self.ABI}_create")
            for name, a in host:
                check(getattr(lib(), f"{self.ABI}_set_param")(lane[0], name.encode(), a.data_ptr(), a.numel()),
                      f"{self.ABI}_set_param({name})")
            check(getattr(lib(), f"{self.ABI}_finalize")(lane[0], None), f"{self.ABI}_finalize")
            lane[1] = sig
        return [lane[0] for lane in self._lanes[:n]]

    @property
    def _handle(self):
        """The lane-0 inference handle, holding the current parameters."""
        return self.lane_handles(1)[0]

    def tiles_entry(self):
        """(ctypes entry, its name) of the fused gather + forward from the uint8 slide (predict_full_patched's launches)."""
        name = f"{self.ABI}_forward_tiles"
        return getattr(lib(), name), name

    @property
    def feature_width(self) -> int:
        """Length of a tile's pooled feature vector, the input of `fc`: 512 (ResNet-18) or 2048 (ResNet-50)."""
        return int(self.fc.in_features)

    def features_entry(self):
        """(ctypes entry, its name) of the fused gather + forward that also stores every tile's pooled features
        (extract_embeddings' launches)."""
        name = f"{self.ABI}_features_tiles"
        return getattr(lib(), name), name

    def default_micro_batch(self) -> int:
        """Tiles per launch of the whole-slide paths: the most one inference launch takes."""
        return self.MAX_TILES

    def _launch_tiles(self, who: str, entry, slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, *out):
        """The argument checks and the one launch of forward_tiles / features_tiles; `out`: the entry's output pointers."""
        if self.training:
            raise NotImplementedError(f"{who} is an inference entry point; call .eval()")
        if not (slide.is_cuda and origins_dev.is_cuda):
            raise RuntimeError("slide and origins must live in GPU memory")
        if slide.dtype != torch.uint8 or slide.dim() != 3 or not slide.is_contiguous():
            raise ValueError("slide must be contiguous uint8[h, w, 3]")
        if origins_dev.dtype != torch.int32 or origins_dev.dim() != 2 or origins_dev.shape[-1] != 2 or not origins_dev.is_contiguous():
            raise ValueError("origins must be contiguous int32[n, 2]")
        h = self.lane_handles(1)[0]
        n = int(origins_dev.shape[0])
        tensors = [None if width is None else torch.empty((n, width), dtype=torch.float32, device=slide.device) for width in out]
        fwd, name = entry()
        check(fwd(h, slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), origins_dev.data_ptr(), n, int(patch),
                  *(None if t is None else t.data_ptr() for t in tensors), _stream(slide.device)), name)
        return tensors

    def forward_tiles(self, slide: torch.Tensor, origins_dev: torch.Tensor, patch: int) -> torch.Tensor:
        """Fused gather + /255 + eval forward straight from the uint8 slide in HBM: one launch, float32[n, n_classes] raw logits."""
        return self._launch_tiles("forward_tiles", self.tiles_entry, slide, origins_dev, patch, self.n_classes)[0]

    def features_tiles(self, slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, return_logits: bool = False):
        """forward_tiles one step earlier: float32[n, feature_width], the global average pool of every tile's last activation (what
        `fc` reads), in one launch; with `return_logits` also the float32[n, n_classes] logits of forward_tiles, bit for bit
        (without it the fc is skipped)."""
        feat, logits = self._launch_tiles("features_tiles", self.features_entry, slide, origins_dev, patch, self.feature_width,
                                          self.n_classes if return_logits else None)
        return (feat, logits) if return_logits else feat

    def cam_entry(self):
        """(ctypes entry, its name) of the fused gather + forward that stores fc applied at every position of the last activation
        (cam.predict_fine_patched's launches)."""
        name = f"{self.ABI}_cam_tiles"
        return getattr(lib(), name), name

    def cam_tiles(self, slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, return_logits: bool = False):
        """The class activation map of every tile in one launch: float32[n, S, S, n_classes], S = patch / 32, fc applied at
        each position of the last activation (position (i, j): the 32 x 32-pixel block of the tile at (32 i, 32 j)); a tile's
        logits are the mean over its positions.  With `return_logits` also the float32[n, n_classes] logits of forward_tiles,
        bit for bit (without it the pooling head is not launched).  `patch` must be a multiple of 32, n_classes <= 64."""
        patch = int(patch)
        if patch <= 0 or patch % 32:
            raise ValueError(f"cam_tiles: patch {patch} is not a multiple of 32 (a position is a 32 x 32-pixel block)")
        if self.n_classes > 64:
            raise ValueError(f"cam_tiles: {self.n_classes} classes, class activation maps take at most 64")
        s = patch // 32
        cam, logits = self._launch_tiles("cam_tiles", self.cam_entry, slide, origins_dev, patch, s * s * self.n_classes,
                                         self.n_classes if return_logits else None)
        cam = cam.view(-1, s, s, self.n_classes)
        return (cam, logits) if return_logits else cam

    def forward_infer(self, x: torch.Tensor) -> torch.Tensor:
        """float32[n, 3, P, P] in [0, 1] on the GPU -> logits through the inference handle (`<ABI>_forward`): the same function as
        forward_tiles on the gathered tiles."""
        x = self._input(x)
        n = int(x.shape[0])
        out = torch.empty((n, self.n_classes), dtype=torch.float32, device=x.device)
        check(getattr(lib(), f"{self.ABI}_forward")(self.lane_handles(1)[0], x.data_ptr(), n, int(x.shape[2]), out.data_ptr(),
                                                    _stream(x.device)), f"{self.ABI}_forward")
        return out

    # ---- forward / training ------------------------------------------------------------------------------
    def _input(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on the GPU only: move the input with .to('cuda')")
        if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
            raise ValueError(f"expected [n, 3, P, P], got {tuple(x.shape)}")
        return x.detach().to(torch.float32).contiguous()

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x: float32[n, 3, P, P] on the GPU (what batch_predictor builds, predict_full_patched.py:67-71) -> float32[n, n_classes]
        raw logits."""
        if not self.training:
            return self._forward_eval(x)
        x = self._input(x)
        if torch.is_grad_enabled():
            return _TrainForward.apply(x, self._engine, *self.parameters())
        return self._engine.forward(x)   # e.g. a train-mode forward under no_grad

    def train_step(self, x, labels, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, group=None, bucket_bytes=DEFAULT_BUCKET_BYTES):
        """Fused step entirely in HIP: forward, CrossEntropy(mean), backward, Adam.
        Under torch.distributed (one process per GPU) the gradients are averaged over `group`: the arena is cut into ~`bucket_bytes`
        buckets in backward-completion order and each bucket's all-reduce starts on a side stream as soon as its last wgrad is
        enqueued (models/patch_cls_simple/ddp.py); Adam waits for the last one (DDP semantics: per-rank batch statistics, replicas
        stay identical).  Returns (loss tensor on device, logits).  nn.Parameters are refreshed lazily by `pull_parameters()` /
        state_dict()."""
        if not self.training:
            raise RuntimeError("train_step needs .train() mode")
        return self._engine.train_step(x, labels, lr, betas, eps, group, bucket_bytes)

    # the trainer's switches and log, kept on the model where callers set and read them
    @property
    def fuse_optimizer(self) -> bool:
        """Single-rank train_step: backward and Adam in one call (False: backward, then adam_step)."""
        return self._engine.fuse_optimizer

    @fuse_optimizer.setter
    def fuse_optimizer(self, value: bool):
        self._engine.fuse_optimizer = value

    @property
    def ddp_wire(self):
        """Gradient wire format of data-parallel steps: None = DH_DDP_WIRE (default f32), "f32", "bf16"."""
        return self._engine.ddp_wire

    @ddp_wire.setter
    def ddp_wire(self, value):
        self._engine.ddp_wire = value

    @property
    def overlap_log(self):
        """(bucket, offset, count) in launch order of the last data-parallel backward."""
        return self._engine.overlap_log

    def flat_gradients(self, device) -> torch.Tensor:
        """The library's whole gradient arena as one float32 tensor view (no copy)."""
        return self._engine.flat(1, device)

    def pull_parameters(self):
        """Library masters and running statistics -> nn.Parameters / buffers (after fused train_step calls)."""
        self._engine.pull_parameters()
        return self

    def state_dict(self, *args, **kwargs):
        self.pull_parameters()
        return super().state_dict(*args, **kwargs)

    def load_state_dict(self, *args, **kwargs):
        """The loaded tensors win over whatever the library holds after fused `train_step` calls (which leave the library's
        masters newer than the nn.Parameters): nothing is pulled back over them, and their new version counters make the next
        training forward push them and the inference handles re-sync."""
        self._engine.native_ahead, self._engine._stats_pending = False, 0
        return super().load_state_dict(*args, **kwargs)
