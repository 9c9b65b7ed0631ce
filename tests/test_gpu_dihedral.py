"""GPU: the eight dihedral views of a resident slide (csrc/dihedral.hip) against NumPy, bit for bit:
view = k + 4 f is np.rot90(np.fliplr(s) if f else s, k).  Random uint8 throughout: a transposition bug hides on smooth data."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = 64                                        # tta.TILE, asserted below
SHAPES = [(1, 1), (1, 300), (300, 1), (37, 53), (T, T), (T - 1, T + 1), (T + 1, 2 * T - 1), (2 * T + 1, 3 * T), (130, 4099),
          (515, 1030)]


@pytest.fixture(scope="module")
def dev(built_lib):
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def view_np(a, v):
    return np.rot90(np.fliplr(a) if v >> 2 else a, v & 3).copy()      # a fresh C-ordered array


def rand(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def test_tile_constant_and_phase_coverage():
    """The shapes are built around the kernel's tile side; 3 w mod 16 (the source pitch, and the destination pitch of the plain
    views) and 3 h mod 16 (the destination pitch of the transposing views) each take at least four values."""
    from deephisto_amd import tta
    assert tta.TILE == T and tta.STORE_GROUP == 16
    assert len({3 * w % 16 for _, w in SHAPES}) >= 4 and len({3 * h % 16 for h, _ in SHAPES}) >= 4


@pytest.mark.parametrize("h,w", SHAPES)
def test_every_view_equals_numpy(dev, h, w):
    from deephisto_amd import tta
    host = rand(h, w, h * 7 + w)
    src = torch.from_numpy(host).to(dev)
    for v, name in enumerate(tta.VIEWS):
        got = tta.dihedral_view(src, name)
        want = view_np(host, v)
        assert tuple(got.shape) == want.shape == (*tta.view_shape(h, w, v), 3) and got.dtype == torch.uint8 and got.is_contiguous()
        assert torch.equal(got.cpu(), torch.from_numpy(want)), (h, w, name)
        assert torch.equal(tta.dihedral_view(src, v).cpu(), torch.from_numpy(want))
    assert torch.equal(src.cpu(), torch.from_numpy(host))            # the source is left alone


def test_round_trips_and_composition(dev):
    from deephisto_amd import tta
    host = rand(131, 77, 3)
    src = torch.from_numpy(host).to(dev)
    views = [tta.dihedral_view(src, v) for v in range(8)]
    for a in range(8):
        assert torch.equal(tta.dihedral_view(views[a], tta.inverse(a)), src), a
        for b in range(8):
            assert torch.equal(tta.dihedral_view(views[a], b), views[tta.compose(a, b)]), (a, b)


def test_guarded_bounds(dev):
    """Source and destination are interior slices of larger buffers filled with a guard byte, starting at odd byte offsets: the
    views are right, and every guard byte is still there, so no store falls outside the image."""
    from deephisto_amd import tta
    guard, lead, tail = 0xA5, 4099, 4096
    for h, w in ((T + 1, 2 * T - 1), (37, 53), (1, 300), (300, 1), (2 * T + 1, 3 * T)):
        n = 3 * h * w
        host = rand(h, w, h + w)
        for so, do in ((lead, lead), (lead + 5, lead + 11)):
            sbuf = torch.full((so + n + tail,), guard, dtype=torch.uint8, device=dev)
            src = sbuf[so:so + n].view(h, w, 3)
            src.copy_(torch.from_numpy(host))
            for v in range(8):
                dbuf = torch.full((do + n + tail,), guard, dtype=torch.uint8, device=dev)
                got = tta.dihedral_view(src, v, out=dbuf[do:do + n])
                assert got.data_ptr() == dbuf.data_ptr() + do
                assert torch.equal(got.cpu(), torch.from_numpy(view_np(host, v))), (h, w, v, so, do)
                flat = dbuf.cpu()
                assert (flat[:do] == guard).all() and (flat[do + n:] == guard).all(), (h, w, v, so, do)
            flat = sbuf.cpu()
            assert (flat[:so] == guard).all() and (flat[so + n:] == guard).all()
            assert torch.equal(src.cpu(), torch.from_numpy(host))


def test_out_is_honoured(dev):
    from deephisto_amd import tta
    host = rand(70, 45, 9)
    src = torch.from_numpy(host).to(dev)
    for shape in ((70 * 45 * 3,), (70, 45, 3), (45, 70, 3), (3, 70 * 45)):
        out = torch.full(shape, 7, dtype=torch.uint8, device=dev)
        got = tta.dihedral_view(src, "r90", out=out)
        assert got.data_ptr() == out.data_ptr() and tuple(got.shape) == (45, 70, 3)
        assert torch.equal(got.cpu(), torch.from_numpy(view_np(host, 1)))


def test_refusals(dev):
    from deephisto_amd import tta
    t = torch.from_numpy(rand(40, 50, 4)).to(dev)
    n = t.numel()
    big = torch.zeros(2 * n, dtype=torch.uint8, device=dev)
    big[:n] = t.view(-1)
    inside = big[:n].view(40, 50, 3)
    for bad in (big[n - 16:2 * n - 16], big[:n]):                               # overlapping `out`
        with pytest.raises(ValueError, match="overlap"):
            tta.dihedral_view(inside, "r90", out=bad)
    with pytest.raises(ValueError, match="overlap"):
        tta.dihedral_view(t, 0, out=t)
    for bad in (torch.empty(n - 1, dtype=torch.uint8, device=dev), torch.empty(n + 1, dtype=torch.uint8, device=dev),      # wrong size
                torch.empty(n, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.uint8),
                torch.empty(2 * n, dtype=torch.uint8, device=dev)[::2]):
        with pytest.raises(ValueError, match="out must be a contiguous uint8 buffer"):
            tta.dihedral_view(t, "r0f", out=bad)
    with pytest.raises(ValueError, match="contiguous"):
        tta.dihedral_view(t[:, ::2], 1)
    with pytest.raises(ValueError, match="contiguous"):
        tta.dihedral_view(t.permute(1, 0, 2), 1)
    with pytest.raises(ValueError, match="must be uint8"):
        tta.dihedral_view(t.to(torch.int16), 1)
    with pytest.raises(ValueError, match=r"uint8\[h, w, 3\]"):
        tta.dihedral_view(t[:, :, :2].contiguous(), 1)
    with pytest.raises(ValueError, match="GPU memory"):
        tta.dihedral_view(t.cpu(), 1)
    with pytest.raises(ValueError, match="unknown view"):
        tta.dihedral_view(t, "r45")
    with pytest.raises(ValueError, match="unknown view"):
        tta.dihedral_view(t, 8)


def test_the_library_refuses_what_python_lets_through(dev, built_lib):
    t = torch.from_numpy(rand(40, 50, 4)).to(dev)
    o = torch.empty_like(t)
    call = built_lib.dh_slide_dihedral
    assert call(t.data_ptr(), 40, 50, 3, o.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert torch.equal(o.view(50, 40, 3).cpu(), torch.from_numpy(view_np(t.cpu().numpy(), 3)))
    for args, word in (((t.data_ptr(), 40, 50, 8, o.data_ptr(), None), b"outside 0..7"),
                       ((t.data_ptr(), 40, 50, -1, o.data_ptr(), None), b"outside 0..7"),
                       ((t.data_ptr(), 0, 50, 1, o.data_ptr(), None), b"bad slide size"),
                       ((t.data_ptr(), 40, -3, 1, o.data_ptr(), None), b"bad slide size"),
                       ((t.data_ptr(), 40, 50, 1, t.data_ptr(), None), b"overlap"),
                       ((t.data_ptr(), 40, 50, 1, t.data_ptr() + 40 * 50 * 3 - 1, None), b"overlap"),
                       ((t.data_ptr() + 1, 39, 50, 1, t.data_ptr(), None), b"overlap"),
                       ((None, 40, 50, 1, o.data_ptr(), None), b"null"),
                       ((t.data_ptr(), 40, 50, 1, None, None), b"null")):
        assert call(*args) == -22 and word in built_lib.dh_last_error(), word


def test_byte_offsets_past_two_to_the_32(dev):
    """A slide of 4.3e9 bytes built from a 1021 x 1031 block (prime sides: an offset that wrapped by 2^31 or 2^32 bytes lands on
    other pixels).  For a mirroring and a transposing view, windows around the pixels at source byte offsets 2^31 and 2^32, and
    the last corner, equal the NumPy view of the same window."""
    from deephisto_amd import tta
    h, w = 40000, 36000
    block = torch.from_numpy(rand(1021, 1031, 5)).to(dev)
    src = block.repeat(40, 35, 1)[:h, :w].contiguous()
    del block
    assert src.numel() > 2 ** 32
    buf = torch.empty(src.numel(), dtype=torch.uint8, device=dev)
    spots = [(edge // (3 * w), edge % (3 * w) // 3) for edge in (2 ** 31, 2 ** 32)] + [(h - 1, w - 1), (0, 0)]
    for v in (2, 1, 7):
        got = tta.dihedral_view(src, v, out=buf)
        for y, x in spots:
            y0, x0 = max(0, min(y - 40, h - 100)), max(0, min(x - 40, w - 100))
            (my, mx), = tta.map_origins([(y0, x0)], h, w, 100, v)
            want = view_np(src[y0:y0 + 100, x0:x0 + 100].cpu().numpy(), v)
            assert torch.equal(got[my:my + 100, mx:mx + 100].cpu(), torch.from_numpy(want)), (v, y, x)
