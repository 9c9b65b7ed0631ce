"""Thin torch-tensor wrappers over the tile-side C ABI (include/deephisto_hip.h).

torch is used only for device memory and streams; every computation below runs
in libdeephisto_hip.so.  No CPU fallbacks: a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import (DH_DTYPE_BF16, DH_DTYPE_F32, DH_LAYOUT_NCHW, DH_LAYOUT_NHWC, check, lib)

_TORCH_DTYPE = {DH_DTYPE_F32: torch.float32, DH_DTYPE_BF16: torch.bfloat16}


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise ValueError(f"{what} must live in GPU memory (got {t.device})")
    if not t.is_contiguous():
        raise ValueError(f"{what} must be contiguous")


def dtype_code(dtype) -> int:
    if dtype in (torch.float32, "f32", "float32", DH_DTYPE_F32):
        return DH_DTYPE_F32
    if dtype in (torch.bfloat16, "bf16", "bfloat16", DH_DTYPE_BF16):
        return DH_DTYPE_BF16
    raise ValueError(f"unsupported dtype {dtype!r}")


def _gather_out(n: int, patch: int, layout: int, dtype, device) -> tuple[torch.Tensor, int]:
    """The output tensor of a gather, (n, 3, P, P) (NCHW) or (n, P, P, 3) in the coded dtype, and the dtype's code."""
    code = dtype_code(dtype)
    shape = (n, 3, patch, patch) if layout == DH_LAYOUT_NCHW else (n, patch, patch, 3)
    return torch.empty(shape, dtype=_TORCH_DTYPE[code], device=device), code


def _host_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _param_rows(dev_t: torch.Tensor, host, n: int, k: int, what: str):
    """Per-tile parameter rows: `dev_t` must be int32[n, k] on the device; returns the optional host copy as a contiguous
    int32[n, k] array for the entry's check (None: not checked)."""
    _require_cuda(dev_t, what)
    if dev_t.dtype != torch.int32 or tuple(dev_t.shape) != (n, k):
        raise ValueError(f"{what} must be int32[{n}, {k}], not {str(dev_t.dtype).replace('torch.', '')}{list(dev_t.shape)}")
    if host is None:
        return None
    host = np.ascontiguousarray(host, dtype=np.int32)
    if host.shape != (n, k):
        raise ValueError(f"{what}_host must be int32[{n}, {k}], not {list(host.shape)}")
    return host


def _stain_table_args(device) -> tuple:
    """(od_dev, od_host, shift, lut_dev, lut_n) of the stain gathers' entries, from the tables of stain.py."""
    from . import stain as S
    od_dev, _, lut, od = S._tables(device)
    return od_dev.data_ptr(), _host_ptr(od), S.APPLY_SHIFT, lut.data_ptr(), S.LUT_SIZE


def tile_grid(h: int, w: int, patch: int, stride: int, batch: int) -> tuple[np.ndarray, int]:
    """(int32[n_padded, 2] (y, x) origins in the reference's order, n_unique).

    Host-side integer work done by dh_tile_grid (full_samplers.py:374-404)."""
    nu, npad = C.c_int64(), C.c_int64()
    check(lib().dh_tile_grid_count(h, w, patch, stride, batch, C.byref(nu), C.byref(npad)), "dh_tile_grid_count")
    out = np.empty((npad.value, 2), dtype=np.int32)
    check(lib().dh_tile_grid(h, w, patch, stride, batch, out.ctypes.data_as(C.c_void_p), npad.value), "dh_tile_grid")
    return out, nu.value


def synth_slide(h: int, w: int, seed: int = 0, device="cuda") -> torch.Tensor:
    """uint8[h, w, 3] closed-form synthetic slide generated directly in HBM."""
    dev = torch.device(device)
    out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
    check(lib().dh_synth_slide(out.data_ptr(), h, w, seed & 0xFFFFFFFF, _stream(dev)), "dh_synth_slide")
    return out


def gather_tiles(slide: torch.Tensor, origins, patch: int, layout: int = DH_LAYOUT_NCHW,
                 dtype=torch.float32, check_bounds: bool = True) -> torch.Tensor:
    """Gather `patch` x `patch` tiles at int32 (y, x) `origins` from a device-resident
    uint8 HWC slide; returns [n,3,P,P] (NCHW) or [n,P,P,3] (NHWC) values k/255."""
    _require_cuda(slide, "slide")
    if slide.dtype != torch.uint8 or slide.dim() != 3 or slide.shape[2] != 3:
        raise ValueError("slide must be uint8[h, w, 3]")
    h, w = int(slide.shape[0]), int(slide.shape[1])
    host = None
    if isinstance(origins, torch.Tensor):
        yx_dev = origins.to(device=slide.device, dtype=torch.int32).contiguous()
        if check_bounds:
            host = np.ascontiguousarray(origins.detach().cpu().numpy().astype(np.int32))
    else:
        host = np.ascontiguousarray(np.asarray(origins, dtype=np.int32).reshape(-1, 2))
        yx_dev = torch.from_numpy(host).to(slide.device)
    n = int(yx_dev.shape[0])
    out, code = _gather_out(n, patch, layout, dtype, slide.device)
    check(lib().dh_tile_gather(slide.data_ptr(), h, w, yx_dev.data_ptr(), _host_ptr(host if check_bounds else None),
                               n, patch, layout, code, out.data_ptr(), _stream(slide.device)), "dh_tile_gather")
    return out


def gather_tiles_aug(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, layout: int = DH_LAYOUT_NCHW,
                     dtype=torch.float32, flip_h: bool = False, flip_v: bool = False) -> torch.Tensor:
    """gather_tiles with the training pipeline's batch-level flips fused in (dh_tile_gather_aug)."""
    _require_cuda(slide, "slide")
    _require_cuda(origins_dev, "origins")
    n = int(origins_dev.shape[0])
    out, code = _gather_out(n, patch, layout, dtype, slide.device)
    check(lib().dh_tile_gather_aug(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), origins_dev.data_ptr(), n,
                                   patch, layout, code, int(flip_h), int(flip_v), out.data_ptr(), _stream(slide.device)),
          "dh_tile_gather_aug")
    return out


def gather_tiles_stain_aug(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, layout: int, dtype, params_dev: torch.Tensor,
                           flip_h: bool = False, flip_v: bool = False, params_host=None) -> torch.Tensor:
    """gather_tiles_aug with a per-tile stain jitter fused in (dh_tile_gather_stain_aug).
    `params_dev`: int32[n, 12] on the device, the rows of stain.jitter_params; `params_host`: the same rows on the host, checked
    by the entry before the launch (None: not checked)."""
    _require_cuda(slide, "slide")
    _require_cuda(origins_dev, "origins")
    n = int(origins_dev.shape[0])
    p_host = _param_rows(params_dev, params_host, n, 12, "params")
    out, code = _gather_out(n, patch, layout, dtype, slide.device)
    check(lib().dh_tile_gather_stain_aug(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), origins_dev.data_ptr(),
                                         params_dev.data_ptr(), _host_ptr(p_host), n, patch, layout, code, int(flip_h), int(flip_v),
                                         *_stain_table_args(slide.device), out.data_ptr(), _stream(slide.device)),
          "dh_tile_gather_stain_aug")
    return out


def gather_tiles_affine_aug(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int, layout: int, dtype, affine_dev: torch.Tensor,
                            flip_h: bool = False, flip_v: bool = False, affine_host=None, params_dev: torch.Tensor | None = None,
                            params_host=None) -> torch.Tensor:
    """gather_tiles_aug with a per-tile rotation and scale about the patch centre fused in, and with `params_dev` the stain
    jitter of gather_tiles_stain_aug as well (dh_tile_gather_affine_aug).  `affine_dev`: int32[n, 4] on
    the device, the rows of geom_aug.affine_params; `affine_host` / `params_host`: the same rows on the host, checked by the
    entry before the launch (None: not checked).  The rotated window shares the patch's centre and reaches up to
    s * P * sqrt(2) / 2 from it; where it leaves the slide it reads 0."""
    _require_cuda(slide, "slide")
    _require_cuda(origins_dev, "origins")
    n = int(origins_dev.shape[0])
    a_host = _param_rows(affine_dev, affine_host, n, 4, "affine")
    p_host = None
    if params_dev is not None:
        p_host = _param_rows(params_dev, params_host, n, 12, "params")
    elif params_host is not None:
        raise ValueError("params_host without params_dev")
    out, code = _gather_out(n, patch, layout, dtype, slide.device)
    stain_args = _stain_table_args(slide.device) if params_dev is not None else (None, None, 0, None, 0)
    check(lib().dh_tile_gather_affine_aug(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), origins_dev.data_ptr(),
                                          params_dev.data_ptr() if params_dev is not None else None, _host_ptr(p_host),
                                          affine_dev.data_ptr(), _host_ptr(a_host), n, patch, layout, code, int(flip_h), int(flip_v),
                                          *stain_args, out.data_ptr(), _stream(slide.device)), "dh_tile_gather_affine_aug")
    return out


class PinnedUploader:
    """Host -> device copies of small per-batch arrays (tile origins, labels) that do not stall the host.

    `torch.from_numpy(a).to(dev)` from pageable memory synchronises the stream: the host cannot prepare batch i+1 while the
    GPU runs step i, and every step starts with an idle GPU.  Here the array is written into one of `depth` pinned staging
    buffers and copied with `non_blocking=True`; an event per slot makes sure a slot is not overwritten before its last
    copy has completed (normally long since)."""

    def __init__(self, device, depth: int = 4):
        self.device, self.depth = torch.device(device), depth
        self._slots: dict = {}   # dtype -> [[pinned byte buffer, event of its last copy] x depth]
        self._next: dict = {}

    def upload(self, arr: "np.ndarray") -> torch.Tensor:
        import numpy as np

        arr = np.ascontiguousarray(arr)
        # one ring per DTYPE, each slot sized to the largest request so far (grown geometrically): arrays whose length changes
        # from batch to batch (per-slide selections of the region samplers) reuse the same pinned memory instead of pinning
        # `depth` new buffers per distinct shape -- pin_memory() is a synchronous hipHostMalloc, the stall this class avoids
        key = arr.dtype.str
        if key not in self._slots:
            self._slots[key] = [[None, None] for _ in range(self.depth)]
            self._next[key] = 0
        k = self._next[key]
        self._next[key] = (k + 1) % self.depth
        slot = self._slots[key][k]
        if slot[1] is not None:
            slot[1].synchronize()
        n = arr.size
        if slot[0] is None or slot[0].numel() < n:
            cap = max(n, 2 * (slot[0].numel() if slot[0] is not None else 0), 64)
            slot[0] = torch.from_numpy(np.empty(cap, dtype=arr.dtype)).pin_memory()
        slot[0].numpy()[:n] = arr.reshape(-1)
        out = slot[0][:n].to(self.device, non_blocking=True).reshape(arr.shape)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        slot[1] = ev
        return out

    def upload_batch(self, origins: "np.ndarray", labels: "np.ndarray") -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """One batch's origins int32[n, 2], labels int64[n] and coordinates float32[n, 2] (= float(origins): exact, |origin| < 2^24,
        what dh_tile_coords_f32 computes) as ONE staged copy: one copy and one event on the stream per batch instead of two copies, two
        events and a kernel.  Returns device views (origins, labels, coords) of the one device buffer."""
        import numpy as np

        n = int(origins.shape[0])
        assert origins.shape == (n, 2) and labels.shape == (n,)
        buf = np.empty(24 * n, np.uint8)
        buf[:8 * n] = np.ascontiguousarray(labels, np.int64).view(np.uint8)                       # 8-byte aligned first
        buf[8 * n:16 * n] = np.ascontiguousarray(origins, np.int32).reshape(-1).view(np.uint8)
        buf[16 * n:] = np.ascontiguousarray(origins, np.float32).reshape(-1).view(np.uint8)
        dev = self.upload(buf)
        return dev[8 * n:16 * n].view(torch.int32).reshape(n, 2), dev[:8 * n].view(torch.int64), dev[16 * n:].view(torch.float32).reshape(n, 2)


def gather_tiles_raw(slide: torch.Tensor, origins_dev: torch.Tensor, patch: int) -> torch.Tensor:
    """float32[n, P, P, 3] of the raw 0..255 pixel values (FullImageRndSampler.generator_torch)."""
    _require_cuda(slide, "slide")
    _require_cuda(origins_dev, "origins")
    n = int(origins_dev.shape[0])
    out, _ = _gather_out(n, patch, DH_LAYOUT_NHWC, torch.float32, slide.device)
    check(lib().dh_tile_gather_raw(slide.data_ptr(), int(slide.shape[0]), int(slide.shape[1]), origins_dev.data_ptr(), n,
                                   patch, out.data_ptr(), _stream(slide.device)), "dh_tile_gather_raw")
    return out


def tile_coords(origins_dev: torch.Tensor) -> torch.Tensor:
    """float32[n, 2] (pos_y, pos_x) from int32 device origins (full_samplers.py:444-451)."""
    _require_cuda(origins_dev, "origins")
    n = int(origins_dev.shape[0])
    out = torch.empty((n, 2), dtype=torch.float32, device=origins_dev.device)
    check(lib().dh_tile_coords_f32(origins_dev.data_ptr(), n, out.data_ptr(), _stream(origins_dev.device)),
          "dh_tile_coords_f32")
    return out


def _origin_rows(origins_host, n: int, rows: str) -> np.ndarray:
    """The host origins of an accumulation as contiguous int32[n, 2]; `rows` names what there are n of."""
    yx = np.ascontiguousarray(np.asarray(origins_host, dtype=np.int32).reshape(-1, 2))
    if yx.shape[0] != n:
        raise ValueError(f"{rows} but {yx.shape[0]} origins")
    return yx


def _sum_canvas(canvas: torch.Tensor | None, shape: tuple, device) -> torch.Tensor:
    """The float32[h//d, w//d, n_cls] canvas of the sums: the caller's, checked, or a new one of zeros."""
    if canvas is None:
        return torch.zeros(shape, dtype=torch.float32, device=device)
    _require_cuda(canvas, "canvas")
    if tuple(canvas.shape) != shape or canvas.dtype != torch.float32:
        raise ValueError("canvas must be float32[h//d, w//d, n_cls]")
    return canvas


def accumulate_logits(logits: torch.Tensor, origins_host: np.ndarray, patch: int, downscale: int,
                      h: int, w: int, canvas: torch.Tensor | None = None,
                      want_map: bool = True) -> tuple[torch.Tensor, torch.Tensor | None]:
    """Ordered accumulation of per-tile logits into the downscaled canvas and argmax
    (examples/predict_full_patched.py:41-62).  Returns (canvas f32[dh,dw,n], map int64[dh,dw])."""
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("logits must be float32[n, n_cls]")
    n, n_cls = int(logits.shape[0]), int(logits.shape[1])
    yx = _origin_rows(origins_host, n, f"{n} logit rows")
    dh_, dw_ = h // downscale, w // downscale
    canvas = _sum_canvas(canvas, (dh_, dw_, n_cls), logits.device)
    cmap = torch.empty((dh_, dw_), dtype=torch.int64, device=logits.device) if want_map else None
    check(lib().dh_accumulate_logits(logits.data_ptr(), yx.ctypes.data_as(C.c_void_p), n, patch, downscale,
                                     n_cls, h, w, canvas.data_ptr(),
                                     cmap.data_ptr() if cmap is not None else None,
                                     _stream(logits.device)), "dh_accumulate_logits")
    return canvas, cmap


def colorize_map(class_map: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    """uint8[h, w, 3]: `colored[pred == id] = color` for every class (predict_full_patched.py:89-95);
    `lut` = uint8[n_cls, 3] indexed by class id, ids without an entry stay black."""
    _require_cuda(class_map, "class_map")
    if class_map.dtype != torch.int64 or not class_map.is_contiguous():
        raise ValueError("class_map must be contiguous int64")
    lut = lut.to(device=class_map.device, dtype=torch.uint8).contiguous()
    out = torch.empty(tuple(class_map.shape) + (3,), dtype=torch.uint8, device=class_map.device)
    check(lib().dh_colorize_map(class_map.data_ptr(), class_map.numel(), lut.data_ptr(), int(lut.shape[0]), out.data_ptr(),
                                _stream(class_map.device)), "dh_colorize_map")
    return out


def overlay_blend(img: torch.Tensor, colored: torch.Tensor, alpha: float = 0.6) -> torch.Tensor:
    """`(img * alpha + colored * (1 - alpha)).astype(uint8)` (predict_full_patched.py:108-110), float64 math."""
    _require_cuda(img, "img")
    _require_cuda(colored, "colored")
    if img.dtype != torch.uint8 or colored.dtype != torch.uint8 or img.shape != colored.shape:
        raise ValueError("img and colored must be uint8 tensors of one shape")
    img, colored = img.contiguous(), colored.contiguous()
    out = torch.empty_like(img)
    check(lib().dh_overlay_blend(img.data_ptr(), colored.data_ptr(), img.numel(), float(alpha), out.data_ptr(),
                                 _stream(img.device)), "dh_overlay_blend")
    return out


def softmax_rows(logits: torch.Tensor) -> torch.Tensor:
    """float32[n, n_cls] per-row softmax (dh_softmax_rows): m = max_c x_c, e_c = expf(x_c - m), s = e_0 + e_1 + ... in class
    order, p_c = e_c / s; n_cls <= 64."""
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("logits must be float32[n, n_cls]")
    out = torch.empty_like(logits)
    check(lib().dh_softmax_rows(logits.data_ptr(), int(logits.shape[0]), int(logits.shape[1]), out.data_ptr(),
                                _stream(logits.device)), "dh_softmax_rows")
    return out


class SlideProbabilities:
    """Per-cell mean softmax probability of a whole-slide prediction, on the device:
    `proba` f32[dh, dw, n_cls], `count` i32[dh, dw] (tiles that covered the cell), `class_map` i64[dh, dw] (first maximum of
    `proba`; `fill_class` where count == 0) and `confidence` f32[dh, dw] (= proba[class_map]; 0 where count == 0).
    While `finished` is False (accumulate_probabilities(..., finish=False)) `proba` holds the running SUMS and `class_map` /
    `confidence` are None: the state to continue from with `state=`; `finish()` ends it in place."""

    def __init__(self, proba: torch.Tensor, count: torch.Tensor, class_map: torch.Tensor | None = None,
                 confidence: torch.Tensor | None = None, fill_class: int = -1):
        self.proba, self.count, self.class_map, self.confidence = proba, count, class_map, confidence
        self.fill_class = int(fill_class)

    @property
    def finished(self) -> bool:
        return self.class_map is not None

    def _outputs(self):
        self.class_map = torch.empty(tuple(self.count.shape), dtype=torch.int64, device=self.count.device)
        self.confidence = torch.empty(tuple(self.count.shape), dtype=torch.float32, device=self.count.device)

    def finish(self, fill_class: int = -1) -> "SlideProbabilities":
        """sums -> mean probabilities in place, class map, confidence (dh_finish_mean)."""
        if self.finished:
            raise ValueError("state is already finished: its sums have been divided by the counts")
        self._outputs()
        self.fill_class = int(fill_class)
        check(lib().dh_finish_mean(self.proba.data_ptr(), self.count.data_ptr(), self.count.numel(), int(self.proba.shape[2]),
                                   self.fill_class, self.proba.data_ptr(), self.class_map.data_ptr(),
                                   self.confidence.data_ptr(), _stream(self.proba.device)), "dh_finish_mean")
        return self


def _proba_state(state: SlideProbabilities | None, dh_: int, dw_: int, n_cls: int, device) -> SlideProbabilities:
    """The unfinished state of a mean accumulation over a dh_ x dw_ canvas: the caller's, checked, or a new one of zeros."""
    if not 1 <= n_cls <= 64:
        raise ValueError(f"n_cls = {n_cls}: the probability kernels take 1 to 64 classes")
    if state is None:
        return SlideProbabilities(torch.zeros((dh_, dw_, n_cls), dtype=torch.float32, device=device),
                                  torch.zeros((dh_, dw_), dtype=torch.int32, device=device))
    if not isinstance(state, SlideProbabilities):
        raise ValueError("state must be a SlideProbabilities")
    if state.finished:
        raise ValueError("state is already finished (its sums were divided): continue from finish=False results only")
    for t, what, dt, shape in ((state.proba, "state.proba", torch.float32, (dh_, dw_, n_cls)),
                               (state.count, "state.count", torch.int32, (dh_, dw_))):
        _require_cuda(t, what)
        if t.dtype != dt or tuple(t.shape) != shape:
            raise ValueError(f"{what} must be {str(dt).replace('torch.', '')}{list(shape)} "
                             f"(canvas h//d x w//d of this call), not {str(t.dtype).replace('torch.', '')}{list(t.shape)}")
    return state


def accumulate_probabilities(logits: torch.Tensor, origins_host: np.ndarray, patch: int, downscale: int, h: int, w: int,
                             state: SlideProbabilities | None = None, fill_class: int = -1,
                             finish: bool = True) -> SlideProbabilities:
    """Softmax of every tile's logits, ordered per-cell sums and hit counts over the footprints of `accumulate_logits` (same
    list, same order, padding duplicates included), then mean = sum / count, its first-maximum class and the confidence
    (dh_softmax_rows, dh_accumulate_mean with the finish fused in).  `state`: an unfinished SlideProbabilities to continue
    from (runs of different patch size chain: all but the last call with finish=False).  An empty list is allowed."""
    _require_cuda(logits, "logits")
    if logits.dtype != torch.float32 or logits.dim() != 2:
        raise ValueError("logits must be float32[n, n_cls]")
    n, n_cls = int(logits.shape[0]), int(logits.shape[1])
    yx = _origin_rows(origins_host, n, f"{n} logit rows")
    state = _proba_state(state, h // downscale, w // downscale, n_cls, logits.device)
    probs = softmax_rows(logits)
    if finish:
        state._outputs()
        state.fill_class = int(fill_class)
    check(lib().dh_accumulate_mean(probs.data_ptr() if n else None, yx.ctypes.data_as(C.c_void_p) if n else None, n, patch,
                                   downscale, n_cls, h, w, state.proba.data_ptr(), state.count.data_ptr(),
                                   state.class_map.data_ptr() if finish else None,
                                   state.confidence.data_ptr() if finish else None, int(fill_class),
                                   _stream(logits.device)), "dh_accumulate_mean")
    return state


# ---- fine maps from class activation maps -----------------------------------------------------------
def expand_positions(origins, patch: int) -> np.ndarray:
    """int32[n * S * S, 2], S = patch / 32: the expanded list that defines the fine accumulation.  Tile-major, positions in order
    p = i * S + j; position (i, j) of the tile at (y, x) is the sub-tile of side 32 at (y + 32 i, x + 32 j).  `accumulate_cam`
    over a tile list is `accumulate_logits` over this list with patch 32 and the rows of the class activation maps."""
    patch = int(patch)
    if patch <= 0 or patch % 32:
        raise ValueError(f"patch {patch} is not a multiple of 32 (a position is a 32 x 32-pixel block)")
    yx = np.asarray(origins, dtype=np.int32).reshape(-1, 2)
    s = patch // 32
    off = 32 * np.stack(np.meshgrid(np.arange(s, dtype=np.int32), np.arange(s, dtype=np.int32), indexing="ij"), axis=-1).reshape(-1, 2)
    return np.ascontiguousarray((yx[:, None, :] + off[None, :, :]).reshape(-1, 2))


def _cam_rows(cam: torch.Tensor, origins_host, patch: int):
    """The argument checks of the fine accumulations: float32[n, S, S, n_cls] (or [n, S * S, n_cls]) rows of n tiles."""
    _require_cuda(cam, "cam")
    patch = int(patch)
    if patch <= 0 or patch % 32:
        raise ValueError(f"patch {patch} is not a multiple of 32 (a position is a 32 x 32-pixel block)")
    s = patch // 32
    if cam.dtype != torch.float32 or cam.dim() not in (3, 4) or int(np.prod(cam.shape[1:-1])) != s * s:
        raise ValueError(f"cam must be float32[n, {s}, {s}, n_cls] for patch {patch}")
    n, n_cls = int(cam.shape[0]), int(cam.shape[-1])
    yx = _origin_rows(origins_host, n, f"class activation maps of {n} tiles")
    return cam.contiguous(), yx, n, n_cls


def accumulate_cam(cam: torch.Tensor, origins_host: np.ndarray, patch: int, downscale: int, h: int, w: int,
                   canvas: torch.Tensor | None = None, want_map: bool = True) -> tuple[torch.Tensor, torch.Tensor | None]:
    """`accumulate_logits` over `expand_positions(origins_host, patch)` with patch 32 and the rows of `cam`
    (float32[n, S, S, n_cls], `ResNetHIP.cam_tiles`), bit for bit, from the tile list's own bin plan (dh_accumulate_cam): every
    tile adds to each cell it covers the row of the one position whose 32-pixel block owns the cell, in tile order.
    Returns (canvas f32[dh, dw, n_cls], map int64[dh, dw])."""
    cam, yx, n, n_cls = _cam_rows(cam, origins_host, patch)
    dh_, dw_ = h // downscale, w // downscale
    canvas = _sum_canvas(canvas, (dh_, dw_, n_cls), cam.device)
    cmap = torch.empty((dh_, dw_), dtype=torch.int64, device=cam.device) if want_map else None
    check(lib().dh_accumulate_cam(cam.data_ptr(), yx.ctypes.data_as(C.c_void_p), n, int(patch), downscale, n_cls, h, w,
                                  canvas.data_ptr(), cmap.data_ptr() if cmap is not None else None, _stream(cam.device)),
          "dh_accumulate_cam")
    return canvas, cmap


def accumulate_cam_probabilities(cam: torch.Tensor, origins_host: np.ndarray, patch: int, downscale: int, h: int, w: int,
                                 fill_class: int = -1) -> SlideProbabilities:
    """`accumulate_probabilities` over the expanded list (`expand_positions`, patch 32, the rows of `cam`), bit for bit: the
    softmax of every position's scores (dh_softmax_rows over n * S * S rows), per-cell sums and hit counts in tile order
    (dh_accumulate_cam_mean), mean, first-maximum class and confidence.  Returns a finished SlideProbabilities."""
    cam, yx, n, n_cls = _cam_rows(cam, origins_host, patch)
    state = _proba_state(None, h // downscale, w // downscale, n_cls, cam.device)
    probs = softmax_rows(cam.view(-1, n_cls))
    state._outputs()
    state.fill_class = int(fill_class)
    check(lib().dh_accumulate_cam_mean(probs.data_ptr() if n else None, yx.ctypes.data_as(C.c_void_p) if n else None, n, int(patch),
                                       downscale, n_cls, h, w, state.proba.data_ptr(), state.count.data_ptr(),
                                       state.class_map.data_ptr(), state.confidence.data_ptr(), int(fill_class),
                                       _stream(cam.device)), "dh_accumulate_cam_mean")
    return state


def heatmap_blend(img: torch.Tensor, field: torch.Tensor, color, alpha: float = 0.6) -> torch.Tensor:
    """`(img * alpha + (float64(field)[..., None] * color) * (1 - alpha)).astype(uint8)` in float64 (dh_heatmap_blend).
    `img` uint8[h, w, 3]; `field` float32[h, w]: one class of the probabilities (`proba[..., k]`, read in place) or the
    confidence; `color`: three values 0..255."""
    _require_cuda(img, "img")
    if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("img must be uint8[h, w, 3]")
    if not field.is_cuda or field.dtype != torch.float32 or tuple(field.shape) != tuple(img.shape[:2]):
        raise ValueError("field must be a float32[h, w] GPU tensor of img's height and width")
    col = np.asarray(color)
    if col.shape != (3,) or (col < 0).any() or (col > 255).any() or (col != np.floor(col)).any():
        raise ValueError(f"color must be three integers in [0, 255], not {color!r}")
    col = np.ascontiguousarray(col, dtype=np.uint8)
    h, w = int(field.shape[0]), int(field.shape[1])
    step = field.stride(1) if w > 1 else 1
    if h * w and (step < 1 or (h > 1 and field.stride(0) != step * w)):   # one class of [h, w, n] is evenly spaced: no copy
        field, step = field.contiguous(), 1
    out = torch.empty_like(img)
    check(lib().dh_heatmap_blend(img.data_ptr(), field.data_ptr(), step, h * w, col.ctypes.data_as(C.c_void_p), float(alpha),
                                 out.data_ptr(), _stream(img.device)), "dh_heatmap_blend")
    return out


class CoverageMap:
    """The device coverage map of FullImageRndSampler (`dh_coverage_*`, csrc/coverage.hip): int32 hit counts [dh, dw]
    at 1/speedup scale, rank -> cell -> origin -> hits per batch.  The narrow interface of coverage.CoveragePlanner:
    `eligible`, `filled`, `size`, `eligible_cells()`, `step(...)` + `counters()`.  Calls go on `stream` (a torch
    stream; default: the device's current stream at construction)."""

    def __init__(self, h: int, w: int, patch: int, speedup: int, dense_level: int, max_batch: int, device="cuda",
                 stream: torch.cuda.Stream | None = None):
        self.device = torch.device(device)
        self.h, self.w, self.P, self.d, self.dl = int(h), int(w), int(patch), int(speedup), int(dense_level)
        self.dh, self.dw = self.h // self.d, self.w // self.d
        self.size = self.dh * self.dw
        self.max_batch = int(max_batch)
        self.stream = stream if stream is not None else torch.cuda.current_stream(self.device)
        self._h = None
        handle = C.c_void_p()
        check(lib().dh_coverage_create(C.byref(handle), self.h, self.w, self.P, self.d, self.dl, self.max_batch,
                                       self._s()), "dh_coverage_create")
        self._h = handle
        self.filled, self.eligible = 0, self.size
        self._last_n, self._last_host = 0, False
        self._host = np.empty((self.max_batch, 2), np.int32)
        self._cells = np.empty(self.max_batch, np.int32)

    def _s(self) -> C.c_void_p:
        return C.c_void_p(self.stream.cuda_stream)

    def step(self, idx, explicit: bool, jitter, origins_dev: int | None = None, host_origins: bool = False):
        """Queue one batch: idx int[n] ranks among the eligible cells (or flat cells when `explicit`), jitter int[n, 2];
        the origins go to the device address `origins_dev` (int32[n, 2]; None: not kept).  Read with counters()."""
        idx = np.ascontiguousarray(idx, dtype=np.int32).ravel()
        jit = np.ascontiguousarray(jitter, dtype=np.int32).reshape(-1)
        n = idx.size
        if jit.size != 2 * n:
            raise ValueError(f"{n} cells but {jit.size} jitter values")
        check(lib().dh_coverage_step(self._h, idx.ctypes.data_as(C.c_void_p), jit.ctypes.data_as(C.c_void_p), n,
                                     1 if explicit else 0, origins_dev, 1 if host_origins else 0, self._s()),
              "dh_coverage_step")
        self._last_n, self._last_host = n, host_origins

    def counters(self):
        """(filled, eligible, int32[n, 2] host origins of the last step or None); waits for the last step's read-back."""
        f, e = C.c_int64(), C.c_int64()
        want = self._last_host and self._last_n > 0
        check(lib().dh_coverage_counters(self._h, C.byref(f), C.byref(e),
                                         self._host.ctypes.data_as(C.c_void_p) if want else None), "dh_coverage_counters")
        self.filled, self.eligible = f.value, e.value
        return self.filled, self.eligible, (self._host[:self._last_n].copy() if want else None)

    def eligible_cells(self) -> np.ndarray:
        """Sorted flat indices of the cells hit fewer than dense_level times (only while there are at most max_batch)."""
        n = C.c_int32()
        check(lib().dh_coverage_eligible_cells(self._h, self._cells.ctypes.data_as(C.c_void_p), self.max_batch,
                                               C.byref(n), self._s()), "dh_coverage_eligible_cells")
        return self._cells[:n.value].astype(np.int64)

    def read_map(self) -> torch.Tensor:
        """float32[dh, dw] copy of the counts on the device (ordered after every queued step)."""
        out = torch.empty((self.dh, self.dw), dtype=torch.float32, device=self.device)
        self.stream.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self.stream):
            check(lib().dh_coverage_read_map(self._h, out.data_ptr(), self._s()), "dh_coverage_read_map")
        torch.cuda.current_stream(self.device).wait_stream(self.stream)
        return out

    def set_map(self, counts: np.ndarray):
        """Test hook (dh_debug_coverage_set_map): replace the counts by int32[dh, dw] and recount."""
        a = np.ascontiguousarray(counts, dtype=np.int32)
        if a.shape != (self.dh, self.dw):
            raise ValueError(f"map must be [{self.dh}, {self.dw}]")
        check(lib().dh_debug_coverage_set_map(self._h, a.ctypes.data_as(C.c_void_p), self._s()), "dh_debug_coverage_set_map")
        self._last_n = 0
        f, e = C.c_int64(), C.c_int64()
        check(lib().dh_coverage_counters(self._h, C.byref(f), C.byref(e), None), "dh_coverage_counters")
        self.filled, self.eligible = f.value, e.value

    def close(self):
        if self._h is not None:
            lib().dh_coverage_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
