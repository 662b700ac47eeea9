"""Host side of the image grids (no GPU): the yardstick tests/grid_ref.py on hand-checked cases, ``hostio.apng_bytes``
against the APNG specification (chunk order, CRCs, sequence numbers, frame contents), the pass-through loader wrapper."""
import struct
import zlib

import numpy as np
import pytest
import torch

from grid_ref import batch_ref, grid_ref, quantise


def test_grid_ref_three_single_pixel_images_written_out():
    # n = 3, H = W = 1, nrow = 2, pad = 1: xmaps = 2, ymaps = 2 -> a 5 x 5 canvas; images at (1,1), (1,3), (3,1); the cell at
    # (3,3) is empty.  Bytes: 0.0 -> 0, 1.0 -> 255, 0.5 -> trunc(128.0) = 128, 0.25 -> trunc(64.25) = 64
    x = np.zeros((3, 3, 1, 1), np.float32)
    x[0, :, 0, 0] = (1.0, 0.5, 0.0)
    x[1, :, 0, 0] = (0.25, 1.0, 1.0)
    x[2, :, 0, 0] = (0.0, 0.0, 1.0)
    z = [0, 0, 0]
    want = np.array([[z, z, z, z, z],
                     [z, [255, 128, 0], z, [64, 255, 255], z],
                     [z, z, z, z, z],
                     [z, [0, 0, 255], z, z, z],
                     [z, z, z, z, z]], np.uint8)
    got = grid_ref(x, nrow=2, padding=1)
    assert got.dtype == np.uint8 and got.shape == (5, 5, 3)
    assert np.array_equal(got, want)
    # pad_value is quantised like a pixel: 0.5 -> 128 everywhere but the three images
    got = grid_ref(x, nrow=2, padding=1, pad_value=0.5)
    image = np.zeros((5, 5, 1), bool)
    image[1, 1] = image[1, 3] = image[3, 1] = True
    assert np.array_equal(got, np.where(image, want, 128).astype(np.uint8))


def test_grid_ref_shapes_and_cells():
    x = np.random.RandomState(0).rand(10, 3, 6, 10).astype(np.float32)
    g = grid_ref(x, nrow=4, padding=2)
    assert g.shape == (3 * 8 + 2, 4 * 12 + 2, 3)                     # ymaps = 3: the last row holds two images
    assert np.array_equal(g[2 + 8:2 + 8 + 6, 2 + 12:2 + 12 + 10], quantise(x[5].transpose(1, 2, 0)))
    assert (g[2 + 16:, 2 + 24:] == 0).all()                         # the two empty cells
    assert (g[:2] == 0).all() and (g[:, :2] == 0).all() and (g[8:10] == 0).all() and (g[:, 12:14] == 0).all()
    # fewer images than nrow: xmaps = n
    assert grid_ref(x[:5], nrow=8).shape == (6 + 4, 5 * 12 + 2, 3)
    # no padding, one per row: the batch form
    assert np.array_equal(grid_ref(x, nrow=1, padding=0).reshape(10, 6, 10, 3), batch_ref(x))


def test_quantise_edges():
    v = np.array([0.0, 1.0, -1.0, 2.0, 0.5 / 255, 1.5 / 255, 254.5 / 255, np.inf, -np.inf], np.float32)
    q = quantise(v)
    assert q[:4].tolist() == [0, 255, 0, 255] and q[-2:].tolist() == [255, 0]
    f = (v[4:7].astype(np.float32) * np.float32(255) + np.float32(0.5))       # two roundings, as torch
    assert q[4:7].tolist() == [int(t) for t in f]


# ---- APNG ----
def _walk(data):
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, chunks = 8, []
    while pos < len(data):
        n, = struct.unpack('>I', data[pos:pos + 4])
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        crc, = struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])
        assert crc == zlib.crc32(tag + body) & 0xffffffff, tag
        chunks.append((tag, body))
        pos += 12 + n
    assert pos == len(data)
    return chunks


def _rows(stream, h, w):
    raw = np.frombuffer(zlib.decompress(stream), np.uint8).reshape(h, 1 + 3 * w)
    assert (raw[:, 0] == 0).all()                                   # filter type 0 on every row
    return raw[:, 1:].reshape(h, w, 3)


def _frames(n, h=5, w=7, seed=0):
    return [np.random.RandomState(seed + i).randint(0, 256, (h, w, 3)).astype(np.uint8) for i in range(n)]


@pytest.mark.parametrize('n', [1, 2, 5])
def test_apng_chunks_follow_the_specification(n):
    from contrad_amd.hostio import apng_bytes
    frames = _frames(n)
    chunks = _walk(apng_bytes(frames, delay_ms=250))
    assert [t for t, _ in chunks] == [b'IHDR', b'acTL', b'fcTL', b'IDAT'] + [b'fcTL', b'fdAT'] * (n - 1) + [b'IEND']
    assert struct.unpack('>IIBBBBB', chunks[0][1]) == (7, 5, 8, 2, 0, 0, 0)
    assert struct.unpack('>II', chunks[1][1]) == (n, 0)
    seq, shown = [], []
    for tag, body in chunks:
        if tag == b'fcTL':
            s, w, h, x0, y0, num, den, dispose, blend = struct.unpack('>IIIIIHHBB', body)
            assert (w, h, x0, y0, num, den, dispose, blend) == (7, 5, 0, 0, 250, 1000, 0, 0)
            seq.append(s)
        elif tag == b'IDAT':
            shown.append(_rows(body, 5, 7))
        elif tag == b'fdAT':
            seq.append(struct.unpack('>I', body[:4])[0])
            shown.append(_rows(body[4:], 5, 7))
    assert seq == list(range(2 * n - 1))
    assert len(shown) == n and all(np.array_equal(a, b) for a, b in zip(shown, frames))


def test_apng_first_frame_is_the_still_png_and_the_cache_changes_nothing():
    from contrad_amd.hostio import apng_bytes, png_bytes
    frames = _frames(3)
    still = _walk(png_bytes(frames[0]))
    anim = _walk(apng_bytes(frames))
    assert [c for c in anim if c[0] in (b'IHDR', b'IDAT', b'IEND')] == still
    cache = []
    a2 = apng_bytes(frames[:2], deflated=cache)
    assert len(cache) == 2 and a2 == apng_bytes(frames[:2])
    assert apng_bytes(frames, deflated=cache) == apng_bytes(frames) and len(cache) == 3


def test_apng_rejects_bad_input():
    from contrad_amd.hostio import apng_bytes
    with pytest.raises(ValueError):
        apng_bytes([])
    with pytest.raises(ValueError):
        apng_bytes(_frames(1) + _frames(1, h=6))
    with pytest.raises(ValueError):
        apng_bytes([np.zeros((4, 4, 3), np.float32)])
    with pytest.raises(ValueError):
        apng_bytes(_frames(1), delay_ms=0)


def test_apng_opens_in_pil():
    Image = pytest.importorskip('PIL.Image')
    import io
    from contrad_amd.hostio import apng_bytes
    frames = _frames(4, h=9, w=6)
    im = Image.open(io.BytesIO(apng_bytes(frames, delay_ms=100)))
    assert im.n_frames == 4 and im.size == (6, 9)
    for i, f in enumerate(frames):
        im.seek(i)
        assert np.array_equal(np.asarray(im.convert('RGB')), f), i


# ---- the monitor's host pieces ----
def test_last_batch_is_a_pass_through():
    from contrad_amd.evaluate.gan import LastBatch
    items = [(torch.full((2,), float(i)), i) for i in range(5)]
    lb = LastBatch(iter(items))
    assert lb.last is None and iter(lb) is lb
    for want in items:
        got = next(lb)
        assert got is want and lb.last is want
    with pytest.raises(StopIteration):
        next(lb)
    assert lb.last is items[-1]

    def endless():
        i = 0
        while True:
            yield i, None
            i += 1
    lb = LastBatch(endless())
    assert [next(lb)[0] for _ in range(4)] == [0, 1, 2, 3] and lb.last == (3, None)


def test_eval_seed_and_fixed_latents_leave_the_global_streams_alone():
    from contrad_amd.evaluate.gan import eval_seed_of, preserved_rng
    torch.manual_seed(1); np.random.seed(1)
    t0, n0 = torch.get_rng_state().clone(), np.random.get_state()[1].copy()
    s = eval_seed_of(7)
    assert s == eval_seed_of(7) and 0 <= s < 10000 and s == int(np.random.RandomState(7).randint(10000))
    with preserved_rng():
        torch.rand(5); np.random.rand(5)
    assert torch.equal(torch.get_rng_state(), t0) and np.array_equal(np.random.get_state()[1], n0)


def test_canvas_shape_is_host_logic():
    from contrad_amd import ops
    assert ops.grid_canvas_shape(16, 32, 32, 4, 2) == (138, 138, 3)
    assert ops.grid_canvas_shape(64, 32, 32, 8, 2) == (274, 274, 3)
    assert ops.grid_canvas_shape(10, 6, 10, 4, 2) == (26, 50, 3)
    assert ops.grid_canvas_shape(5, 3, 5, 8, 2) == (7, 37, 3)
    assert ops.grid_canvas_shape(7, 5, 3, 1, 0) == (35, 3, 3)


def test_entry_rejects_bad_arguments_without_gpu():
    from contrad_amd import _lib
    lib = _lib.lib()
    buf = (np.zeros(64, np.float32), np.zeros(64, np.uint8))
    src, dst = buf[0].ctypes.data, buf[1].ctypes.data
    for args in ((None, dst, 1, 1, 1, 1, 0), (src, None, 1, 1, 1, 1, 0), (src, dst, 0, 1, 1, 1, 0), (src, dst, 1, 0, 1, 1, 0),
                 (src, dst, 1, 1, 0, 1, 0), (src, dst, 1, 1, 1, 0, 0), (src, dst, 1, 1, 1, 1, -1), (src + 2, dst, 1, 1, 1, 1, 0),
                 (src, dst + 1, 1, 1, 1, 1, 0), (src, dst, 2 ** 31 - 1, 2 ** 20, 1, 1, 0)):
        assert lib.raw('contrad_image_grid_u8')(*args, 0.0, None) == -22, args
