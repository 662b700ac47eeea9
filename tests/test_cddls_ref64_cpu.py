"""cDDLS sampling without a GPU: the float64 restatement (tests/cddls_ref64.py) against the reference's own
``_sample_cddls`` (tests/golden/cddls.npz), the numpy Philox4x32-10 against known answers, the host pieces of
contrad_amd/cddls.py, the declared C ABI."""
import os
import re
import struct
import zlib

import numpy as np
import pytest
import torch

import cddls_ref64 as R
from conftest import GOLDEN, ROOT

@pytest.fixture(scope='module')
def fx():
    return np.load(os.path.join(GOLDEN, 'cddls.npz'))


def relmax(a, b):
    return float((a - b).abs().max() / b.abs().max())


@pytest.mark.parametrize('y', [3, 7])
def test_ref64_reproduces_reference(fx, y):
    """Increments, not states (the states are dominated by z0).  Relative max error < 1e-10: float64 round-off through
    ~20 layers with K <= 8192 is of order 1e-13.  The networks are NOT the ones of the other sndcgan fixtures: same
    det_fill seeds, plus five power iterations on D's spectral-norm vectors (cddls_ref64.fixture_networks says why)."""
    steps, images = R.ref_trajectory(fx, y)
    zs = torch.from_numpy(fx['y%d.z' % y])
    prev = torch.from_numpy(fx['z0'].astype(np.float64))
    for k, st in enumerate(steps):
        assert relmax(st['z'] - st['z_prev'], zs[k] - prev) < 1e-10, k
        prev = zs[k]
        assert abs(st['e'].sum().item() - fx['y%d.e_sum' % y][k]) < 1e-10 * abs(fx['y%d.e_sum' % y][k])
        s_ref = torch.from_numpy(fx['y%d.z2_sums' % y])
        assert relmax(st['z2'].reshape(4, -1).sum(1) - st['z2_prev'].reshape(4, -1).sum(1), s_ref[k + 1] - s_ref[k]) < 1e-10
    z2_first = torch.from_numpy(fx['z2_0'].astype(np.float64))
    assert relmax(steps[-1]['z2'] - z2_first, torch.from_numpy(fx['y%d.z2_last' % y]) - z2_first) < 1e-10
    assert relmax(images, torch.from_numpy(fx['y%d.images' % y])) < 1e-10


def test_eval_generator_matches_oracle():
    gsd, _ = R.fixture_networks()
    z = torch.rand(3, 128, dtype=torch.float64, generator=torch.Generator().manual_seed(1)) * 2 - 1
    assert torch.equal(R.g_eval_forward(gsd, z), R.O.sndcgan_g_forward(gsd, z, training=False))


def test_philox_known_answers():
    def run(ctr, key):
        return ['%08x' % v for v in R.philox4x32_10(np.array([ctr], np.uint64), key)[0]]
    assert run([0, 0, 0, 0], (0, 0)) == ['6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']
    f = 0xffffffff
    assert run([f, f, f, f], (f, f)) == ['408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd']
    assert run([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], (0xa4093822, 0x299f31d0)) == \
        ['d16cfe09', '94fdcceb', '5001e420', '24126ea1']


def test_counter_layout():
    """Element e reads word e % 4 of counter (e // 4, step, stream, 0); the key is the seed's two halves."""
    seed = (0x299f31d0 << 32) | 0xa4093822
    w = R.philox_words(11, seed, 2, 9)
    for e in (0, 5, 10):
        assert w[e] == R.philox4x32_10(np.array([[e // 4, 9, 2, 0]], np.uint64), (0xa4093822, 0x299f31d0))[0][e % 4]
    assert len(R.normals64(7, 1, 0, 0)) == 7 and np.array_equal(R.normals64(7, 1, 0, 0), R.normals64(8, 1, 0, 0)[:7])


def test_numpy_generator_statistics():
    """The bounds the GPU test asserts hold for the numpy generator itself at the same seeds."""
    a, b, c, d = (R.normals64(R.STAT_N, *t) for t in (R.STAT_A, R.STAT_B, R.STAT_STEP, R.STAT_SEED2))
    for x in (a, b):
        m1, m2, m4 = R.moments(x)
        assert m1 < R.B_MEAN and m2 < R.B_VAR and m4 < R.B_M4, (m1, m2, m4)
    assert R.corr(a, b) < R.B_CORR and R.corr(a, c) < R.B_CORR and R.corr(a, d) < R.B_CORR
    assert np.abs(a).max() < 5.9            # sqrt(-2 ln 2^-25) = 5.887: the largest radius a 24-bit uniform gives


def test_float32_box_muller_restatement():
    """The kernel's float32 Box-Muller arithmetic, restated in numpy, stays within the bound the GPU test asserts (1.6e-5:
    32 ulp at 5.9), also where a rounded uniform would fail: words whose 24-bit uniform is next to 1 (radius ~ 2.4e-4)."""
    w = R.philox_words(R.STAT_N, *R.STAT_A)
    assert np.abs(R.box_muller32(w).astype(np.float64) - R.box_muller64(w)).max() < 1.6e-5
    edge = np.array([0xffffff00, 0x40000000, 0xfffffe00, 0xc0000000, 0x00000000, 0x00000000, 0x7fffff00, 0x80000000], np.uint32)
    assert np.abs(R.box_muller32(edge).astype(np.float64) - R.box_muller64(edge)).max() < 1.6e-5
    assert abs(R.box_muller64(edge)[1]) > 2e-4          # a uniform rounded to 1.0 would give radius 0 here


def test_cli_defaults_and_plan():
    from contrad_amd import cddls
    P = cddls.parse_args(['logdir', 'lin.pth.tar', 'sndcgan'])
    assert (P.lbd, P.n_steps, P.eps, P.sigma_n, P.n_samples, P.n_classes, P.batch_size) == (1.0, 1000, 0.01, 0.1, 10000, 10, 500)
    assert isinstance(P.n_steps, int) and isinstance(cddls.parse_args(['a', 'b', 'c', '--n_steps', '7']).n_steps, int)
    assert (P.seed, P.graph, P.log_energy) == (None, False, False)
    plan = cddls.batch_plan(10000, 10, 500)
    assert len(plan) == 20 and plan[3] == (1, 1, 1500, 500) and sum(p[3] for p in plan) == 10000
    # n_samples not divisible by n_classes * batch_size: index = y * (n_samples // n_classes) + i * batch_size + j
    plan = cddls.batch_plan(12, 2, 4)
    assert plan == [(0, 0, 0, 4), (0, 1, 4, 2), (1, 0, 6, 4), (1, 1, 10, 2)]
    idx = [off + j for (_, _, off, keep) in plan for j in range(keep)]
    assert idx == list(range(12))
    plan = cddls.batch_plan(13, 3, 5)           # 4 per class, one batch each, the 13th image is never made
    assert plan == [(0, 0, 0, 4), (1, 0, 4, 4), (2, 0, 8, 4)]
    assert all(off + keep <= 13 for (_, _, off, keep) in plan)


@pytest.mark.parametrize('hb', [4, 2])
def test_class_row_permutation(hb):
    from contrad_amd.cddls import permute_class_row
    g = torch.Generator().manual_seed(hb)
    f = torch.randn(3, 512 * hb * hb, generator=g)          # NCHW-flattened features, as the checkpoint's head reads them
    w = torch.randn(512 * hb * hb, generator=g)
    f_nhwc = f.view(3, 512, hb, hb).permute(0, 2, 3, 1).reshape(3, -1)
    assert torch.allclose(f_nhwc @ permute_class_row(w, hb, hb), f @ w, rtol=0, atol=1e-3)
    assert torch.equal(permute_class_row(w, hb, hb).view(hb, hb, 512).permute(2, 0, 1).reshape(-1), w)


def _decode_png(data):
    """Minimal PNG decoder (8-bit RGB, non-interlaced, all five filter types)."""
    assert data[:8] == b'\x89PNG\r\n\x1a\n'
    pos, idat, hdr = 8, b'', None
    while pos < len(data):
        n, tag = struct.unpack('>I', data[pos:pos + 4])[0], data[pos + 4:pos + 8]
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack('>I', data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xffffffff
        if tag == b'IHDR':
            hdr = struct.unpack('>IIBBBBB', body)
        elif tag == b'IDAT':
            idat += body
        pos += 12 + n
    w, h, depth, ctype, comp, flt, lace = hdr
    assert (depth, ctype, comp, flt, lace) == (8, 2, 0, 0, 0)
    raw = zlib.decompress(idat)
    stride, out, prev = 3 * w, np.zeros((h, 3 * w), np.uint8), np.zeros(3 * w, np.int64)
    for r in range(h):
        ft, line = raw[r * (stride + 1)], np.frombuffer(raw[r * (stride + 1) + 1:(r + 1) * (stride + 1)], np.uint8).astype(np.int64)
        cur = np.zeros(stride, np.int64)
        for i in range(stride):
            a = cur[i - 3] if i >= 3 else 0
            b, c = prev[i], (prev[i - 3] if i >= 3 else 0)
            pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
            pred = [0, a, b, (a + b) // 2, a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)][ft]
            cur[i] = (line[i] + pred) & 255
        out[r], prev = cur, cur
    return out.reshape(h, w, 3)


def test_png_roundtrip(tmp_path):
    from contrad_amd.hostio import png_bytes, to_uint8, write_png
    img = np.random.RandomState(0).randint(0, 256, (9, 13, 3)).astype(np.uint8)
    assert np.array_equal(_decode_png(png_bytes(img)), img)
    write_png(str(tmp_path / 'a.png'), img)
    assert np.array_equal(_decode_png((tmp_path / 'a.png').read_bytes()), img)
    try:
        from PIL import Image
    except ImportError:
        Image = None
    if Image is not None:
        assert np.array_equal(np.asarray(Image.open(str(tmp_path / 'a.png')).convert('RGB')), img)
    # save_image's quantisation: x * 255 + 0.5, clamp, truncate
    x = torch.tensor([-0.1, 0.0, 0.5 / 255 - 1e-4, 0.5 / 255 + 1e-4, 0.5, 1.0, 1.2])
    assert to_uint8(x).tolist() == [0, 0, 0, 1, 128, 255, 255]
    with pytest.raises(ValueError):
        png_bytes(np.zeros((4, 4), np.uint8))


def test_abi_symbols():
    from contrad_amd._lib import HEADER_PATH, lib, parse_header
    names = ['contrad_cddls_normal_fill', 'contrad_cddls_feature_seed', 'contrad_cddls_bn_relu_bwd_eval',
             'contrad_cddls_compose', 'contrad_cddls_image_end', 'contrad_cddls_latent_update', 'contrad_cddls_energy']
    protos = parse_header(HEADER_PATH)
    src = open(os.path.join(ROOT, 'contrad_amd', 'csrc', 'cddls.hip')).read()
    for n in names:
        assert n in protos and re.search(r'extern "C" int %s\(' % n, src), n
        assert lib().raw(n) is not None
    assert lib().raw('contrad_abi_version')() == 3
    assert 'getenv' not in src
