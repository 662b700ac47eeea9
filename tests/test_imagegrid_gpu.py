"""csrc/imagegrid.hip against tests/grid_ref.py: the outputs are bytes, so every comparison is exact."""
import numpy as np
import pytest
import torch

from grid_ref import batch_ref, grid_ref

pytestmark = pytest.mark.gpu

DEV = 'cuda'
# (n, H, W, nrow, pad)
SHAPES = [(1, 1, 1, 8, 2), (5, 3, 5, 8, 2), (10, 6, 10, 4, 2), (64, 32, 32, 8, 2), (16, 32, 32, 4, 2), (7, 5, 3, 1, 0)]


def boundary_set():
    """For k = 0..256 the floats within +-8 ulps of float32((k - 0.5) / 255): where trunc(x * 255 + 0.5) steps from k - 1 to
    k, and the two clamp edges.  17 * 257 = 4369 values."""
    c = (np.arange(257, dtype=np.float64) - 0.5) / 255.0
    bits = c.astype(np.float32).view(np.int32).astype(np.int64)
    # ulp steps on the sign-magnitude bit pattern: map to a monotone integer line, step, map back
    line = np.where(bits < 0, -(bits & 0x7fffffff), bits)
    out = []
    for d in range(-8, 9):
        v = line + d
        out.append(np.where(v < 0, (-v) | 0x80000000, v).astype(np.uint32).view(np.float32))
    vals = np.stack(out, 1).reshape(-1)
    assert vals.size == 4369 and np.isfinite(vals).all()
    return vals


def _values(kind, shape, seed=0):
    rs = np.random.RandomState(seed)
    n = int(np.prod(shape))
    if kind == 'uniform':
        x = rs.uniform(-0.25, 1.25, n).astype(np.float32)
    elif kind == 'boundary':
        x = np.resize(boundary_set(), n)
    elif kind == 'inf':
        x = rs.uniform(-0.25, 1.25, n).astype(np.float32)
        x[rs.rand(n) < 0.1] = np.inf
        x[rs.rand(n) < 0.1] = -np.inf
    return torch.from_numpy(x.reshape(shape))


def test_boundary_set_brackets_every_step():
    from grid_ref import quantise
    q = quantise(boundary_set()).reshape(257, 17).astype(int)
    k = np.arange(257)
    assert (q[:, 0] == np.clip(k - 1, 0, 255)).all() and (q[:, -1] == np.clip(k, 0, 255)).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_grid_matches_the_yardstick_on_uniform_values(shape):
    from contrad_amd import ops
    n, H, W, nrow, pad = shape
    x = _values('uniform', (n, 3, H, W), seed=n)
    got = ops.image_grid_u8(x.to(DEV), nrow=nrow, padding=pad)
    want = grid_ref(x, nrow, pad)
    assert got.dtype == torch.uint8 and tuple(got.shape) == want.shape == ops.grid_canvas_shape(n, H, W, nrow, pad)
    assert np.array_equal(got.cpu().numpy(), want)


@pytest.mark.parametrize('pad_value', [0.5, 1.0])
def test_pad_value_is_quantised_like_a_pixel(pad_value):
    from contrad_amd import ops
    x = _values('uniform', (3, 3, 8, 8), seed=3)
    got = ops.image_grid_u8(x.to(DEV), nrow=2, padding=1, pad_value=pad_value).cpu().numpy()
    assert np.array_equal(got, grid_ref(x, 2, 1, pad_value))
    assert got[0, 0, 0] == (128 if pad_value == 0.5 else 255) and (got[10:, 10:] == got[0, 0, 0]).all()     # frame, empty cell


@pytest.mark.parametrize('kind', ['boundary', 'inf'])
@pytest.mark.parametrize('shape', [(64, 32, 32, 8, 2), (16, 32, 32, 4, 2), (7, 5, 3, 1, 0)], ids=lambda s: 'x'.join(map(str, s)))
def test_truncation_and_clamp_edges(shape, kind):
    from contrad_amd import ops
    n, H, W, nrow, pad = shape
    x = _values(kind, (n, 3, H, W), seed=7)
    got = ops.image_grid_u8(x.to(DEV), nrow=nrow, padding=pad).cpu().numpy()
    assert np.array_equal(got, grid_ref(x, nrow, pad))


@pytest.mark.parametrize('kind', ['uniform', 'boundary', 'inf'])
def test_batch_form_matches_to_uint8(kind):
    from contrad_amd import ops
    from contrad_amd.hostio import to_uint8
    for shape in ((7, 3, 5, 3), (16, 3, 32, 32)):                   # 105 pixels: a scalar tail of one; 16384: none
        x = _values(kind, shape, seed=11)
        got = ops.images_u8(x.to(DEV))
        assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], shape[2], shape[3], 3)
        assert np.array_equal(got.cpu().numpy(), batch_ref(x))
        assert torch.equal(got, to_uint8(x.to(DEV)).permute(0, 2, 3, 1).contiguous())      # the chain it replaces


def test_nan_is_written_as_zero():
    from contrad_amd import ops
    rs = np.random.RandomState(5)
    x = rs.uniform(0.1, 0.9, (6, 3, 5, 7)).astype(np.float32)
    nan = rs.rand(*x.shape) < 0.2
    x[nan] = np.nan
    x[0, 0, 0, 0] = -np.nan
    nan[0, 0, 0, 0] = True
    got = ops.images_u8(torch.from_numpy(x).to(DEV)).cpu().numpy()
    assert (got[nan.transpose(0, 2, 3, 1)] == 0).all()
    assert (got[~nan.transpose(0, 2, 3, 1)] >= 26).all()             # every other byte: a pixel of [0.1, 0.9]
    clean = np.where(nan, 0.0, x).astype(np.float32)
    assert np.array_equal(got, batch_ref(clean))
    # a NaN pad_value: the frame is 0, the images are not disturbed
    g = ops.image_grid_u8(torch.from_numpy(clean).to(DEV), nrow=4, padding=2, pad_value=float('nan')).cpu().numpy()
    assert np.array_equal(g, grid_ref(clean, 4, 2, 0.0))


@pytest.mark.parametrize('shape', [(10, 6, 10, 4, 2), (7, 5, 3, 1, 0), (16, 32, 32, 4, 2)], ids=lambda s: 'x'.join(map(str, s)))
def test_unaligned_source_canaries_and_repeatability(shape):
    from contrad_amd import ops
    n, H, W, nrow, pad = shape
    x = _values('uniform', (n, 3, H, W), seed=13)
    big = torch.empty(x.numel() + 1, device=DEV)
    src = big[1:].view(n, 3, H, W)                                  # base 4 bytes behind a 16-byte aligned address
    src.copy_(x)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    cshape = ops.grid_canvas_shape(n, H, W, nrow, pad)
    size = int(np.prod(cshape))
    outs = []
    for fill in (0xA5, 0x5A):
        buf = torch.full((64 + size + 64,), fill, dtype=torch.uint8, device=DEV)
        out = buf[64:64 + size].view(cshape)
        assert ops.image_grid_u8(src, nrow=nrow, padding=pad, out=out).data_ptr() == out.data_ptr()
        b = buf.cpu().numpy()
        assert (b[:64] == fill).all() and (b[64 + size:] == fill).all()
        outs.append(b[64:64 + size].reshape(cshape))
    assert np.array_equal(outs[0], outs[1])                         # every byte written, whatever was there before
    assert np.array_equal(outs[0], grid_ref(x, nrow, pad))
    assert torch.equal(ops.image_grid_u8(src, nrow=nrow, padding=pad), ops.image_grid_u8(src, nrow=nrow, padding=pad))


def test_wrappers_reject_what_the_kernel_does_not_take():
    from contrad_amd import ops
    x = torch.rand(4, 3, 8, 8, device=DEV)
    bad = [x.double(), x.half(), (x * 255).to(torch.uint8), x.permute(0, 1, 3, 2), x[:, :, :, ::2], x[:, :2], torch.rand(4, 4, 8, 8, device=DEV),
           torch.rand(4, 1, 8, 8, device=DEV), x[0], x.cpu(), x[:0], x.cpu().numpy()]
    for fn in (ops.image_grid_u8, ops.images_u8):
        for t in bad:
            with pytest.raises(RuntimeError):
                fn(t)
    with pytest.raises(ValueError):
        ops.image_grid_u8(x, nrow=0)
    with pytest.raises(ValueError):
        ops.image_grid_u8(x, padding=-1)
    for out in (torch.empty(12, 42, 3, device=DEV), torch.empty(12, 42, 4, dtype=torch.uint8, device=DEV),
                torch.empty(12, 42, 3, dtype=torch.uint8), torch.empty(12 * 42 * 3 + 1, dtype=torch.uint8, device=DEV)[1:].view(12, 42, 3)):
        with pytest.raises(RuntimeError):
            ops.image_grid_u8(x, nrow=4, padding=2, out=out)


def test_evaluators_keep_the_reference_interface():
    from contrad_amd.evaluate.gan import FixedSampleGeneration, ImageGrid
    from contrad_amd.models.gan import get_architecture
    x = torch.rand(70, 3, 32, 32, device=DEV)
    ig = ImageGrid()
    with pytest.raises(ValueError):
        ig.value
    g1, g2 = ig.update(1, x), ig.update(2, x.flip(0))
    assert isinstance(g1, np.ndarray) and g1.dtype == np.uint8 and g1.shape == (274, 274, 3)
    assert np.array_equal(g1, grid_ref(x[:64].cpu(), 8, 2)) and ig.value is g2 and len(ig.summary()) == 2
    vol = ImageGrid(volatile=True)
    vol.update(1, x); vol.update(2, x)
    assert len(vol.summary()) == 1
    ig.reset()
    assert ig.summary() == []
    torch.manual_seed(0)
    G, _ = get_architecture('sndcgan', (32, 32, 3))
    G = G.to(DEV).eval()
    for p in G.parameters():
        p.requires_grad_(False)
    state = torch.get_rng_state().clone()
    fg = FixedSampleGeneration(G, seed=12)
    assert torch.equal(torch.get_rng_state(), state)                # seeded latents: the global stream is not read
    a, b = fg.update(1), fg.update(2)
    assert a.shape == (138, 138, 3) and np.array_equal(a, b) and len(fg.summary()) == 2
    with torch.no_grad():
        assert np.array_equal(a, grid_ref(G(fg._latent).cpu(), 4, 2))
    ref_style = FixedSampleGeneration(G)                            # the reference's constructor: G.sample_latent(16)
    assert not torch.equal(torch.get_rng_state(), state) and ref_style._latent.shape == (16, 128)
