"""The cases behind tests/golden/embed_tile_bits.npz: inputs from an integer hash and one walk over the three entry points that run
the 32 x 64 tile of deephisto_amd/csrc/embed.hip (dh_embed_scores, dh_embed_assign, dh_embed_project), through a ctypes handle.

tools/embed_bits.py records the arrays of `run` from a library of its choice; tests/test_gpu_embed_bits.py compares the tree's
library with them bit for bit.  Both call `run`, so both see the same inputs: integers mixed by shifts and multiplications modulo
2^32 and mapped to float32 in [-0.5, 0.5] -- no random generator and no libm, hence nothing a NumPy version could change.

n = 38 is one full 32-row tile and 6 rows of a second; D = 128 is two LDS stages (the prefetch and its last-stage edge), D = 64
one stage without a prefetch (the first 64 columns, made contiguous).  K = 1 leaves 15 of 16 threads idle, K = 17 puts one
member into the second prototype group, K = 64 fills the tile; K = 5 of the assignment runs the rows-per-lane kernel instead."""
import ctypes as C

import numpy as np

N, DS = 38, (128, 64)
SCORE_KS, ASSIGN_KS = (1, 17, 64), (5, 17, 64)
SCORE_SCALE = -1.5
SENTINEL = 7.0   # what project's output holds before the call: the columns behind K keep it


def hashed(rows, cols, salt):
    """float32[rows, cols] in [-0.5, 0.5]: element (i, c) from the integer (i + salt) * 2654435761 + c * 40503, mixed, over 2^32."""
    i = np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(salt)
    c = np.arange(cols, dtype=np.uint64)[None, :]
    m = np.uint64(0xFFFFFFFF)
    h = (i * np.uint64(2654435761) + c * np.uint64(40503)) & m
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(2246822519)) & m
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(3266489917)) & m
    h ^= h >> np.uint64(16)
    return (h.astype(np.float64) / 2.0 ** 32 - 0.5).astype(np.float32)


def inputs(D):
    """(x float32[38, D], p float32[64, D], q float32[17, D], mean float32[D], scale float32[64]): rows, prototypes / centres /
    components (the first K rows of p), the centres of the merge pass, and project's mean and per-component scale."""
    x, p, q = hashed(N, 128, 0)[:, :D], hashed(64, 128, 1000)[:, :D], hashed(17, 128, 2000)[:, :D]
    mean = (0.25 * hashed(1, 128, 3000)[0, :D]).astype(np.float32)
    scale = (hashed(1, 64, 4000)[0] + np.float32(1.25)).astype(np.float32)
    return tuple(np.ascontiguousarray(a) for a in (x, p, q, mean, scale))


def ld_of(K):
    """project's output row: K rounded up to a multiple of four, K = 17 into 20."""
    return -(-K // 4) * 4


def run(lib, torch, dev):
    """{name: array}: every recorded output, from the library behind the ctypes handle `lib` on device `dev`."""
    out = {}
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def ptr(t):
        return C.c_void_p(t.data_ptr())

    def call(name, *args):
        rc = getattr(lib, name)(*args, stream)
        assert rc == 0, f"{name} returned {rc}"

    for D in DS:
        x, p, q, mean, scale = (torch.from_numpy(a).to(dev) for a in inputs(D))
        for K in SCORE_KS:
            s = torch.empty((N, K), dtype=torch.float32, device=dev)
            call("dh_embed_scores", ptr(x), C.c_int64(N), C.c_int32(D), ptr(p), C.c_int32(K), C.c_float(SCORE_SCALE), ptr(s))
            out[f"scores_D{D}_K{K}"] = s.cpu().numpy()
            ld = ld_of(K)
            o = torch.full((N, ld), SENTINEL, dtype=torch.float32, device=dev)
            call("dh_embed_project", ptr(x), C.c_int64(N), C.c_int32(D), ptr(mean), ptr(p), C.c_int32(K), ptr(scale), ptr(o),
                 C.c_int32(ld))
            out[f"project_D{D}_K{K}"] = o.cpu().numpy()
        for K in ASSIGN_KS + ("merge",):
            lab = torch.full((N,), -7, dtype=torch.int32, device=dev)
            dist = torch.full((N,), -1.0, dtype=torch.float32, device=dev)
            passes = [(p, 64, 0, 0), (q, 17, 64, 1)] if K == "merge" else [(p, K, 0, 0)]
            for c, k, k0, merge in passes:
                call("dh_embed_assign", ptr(x), C.c_int64(N), C.c_int32(D), ptr(c), C.c_int32(k), C.c_int32(k0), C.c_int32(merge),
                     ptr(lab), ptr(dist))
            out[f"assign_label_D{D}_K{K}"] = lab.cpu().numpy()
            out[f"assign_dist_D{D}_K{K}"] = dist.cpu().numpy()
    torch.cuda.synchronize(dev)
    return out
