"""The layer under the evaluators of a frozen discriminator's penultimate features (knn.py, prdc.py, kid.py, nearest.py; DESIGN.md
section 15): images to normalised feature rows, rows to banks, banks to similarity chunks, and the checkpoints, image
sets and command line that the evaluators of "a real set against a fake set" share.

  * features: ``D.penultimate`` under ``no_grad`` in eval mode (no power iteration, no augmentation), rows L2-normalised
    by ``contrad_l2norm_fwd`` (x / max(||x||, 1e-12), F.normalize's rule);
  * the bank layout: a bank of n rows is kept transposed, [d][n_pad] with n_pad = round_up(n, 4) and zero padding
    columns -- the packed weight layout of the conv engine, so ``S = Q bank^T`` is ``ops.conv2d_fwd`` on a (m, 1, 1, d) input;
  * the chunk rule: ``S`` is made ``chunk_rows_of(n_pad)`` = max(1, min(MAX_CHUNK_ROWS, S_CHUNK_FLOATS // n_pad)) query rows
    at a time, at most 64 MB: the GEMM writes a chunk and one kernel of the evaluator reads it while it is still cached.
    ``similarity_chunks`` is the one loop that does this.
"""
import json
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import ops
from .evaluate.gan import fixed_latent, freeze, preserved_rng
from .models.gan import get_architecture

S_CHUNK_FLOATS = 1 << 24          # one chunk of S: 64 MB
MAX_CHUNK_ROWS = 512


# ---- rows and banks ----
def normalize_rows(feats):
    """x / max(||x||_2, 1e-12) per row of a CUDA fp32 (n, d) matrix (contrad_l2norm_fwd)."""
    if feats.dim() != 2:
        raise RuntimeError('features: rows must be an (n, d) matrix, got %s' % (tuple(feats.shape),))
    if feats.stride(-1) != 1:
        feats = feats.contiguous()
    return ops.l2norm_fwd(feats)[0]


def new_bank(n, d, device):
    """The transposed bank [d][round_up(n, 4)], zero-filled (the padding columns stay zero)."""
    return torch.zeros(d, ops.round_up(n, 4), device=device, dtype=torch.float32)


def bank_of(rows):
    """The transposed bank [d][round_up(n, 4)] of normalised rows [n, d]."""
    n, d = rows.shape
    bankT = new_bank(n, d, rows.device)
    bankT[:, :n].copy_(rows.t())
    return bankT


# ---- similarities ----
def chunk_rows_of(n_pad):
    return max(1, min(MAX_CHUNK_ROWS, S_CHUNK_FLOATS // n_pad))


def similarities(q, bankT, out):
    """out[m][n_pad] = q[m][d] bank^T on the conv engine (a linear layer whose packed weight is the bank)."""
    m, (d, n_pad) = q.shape[0], bankT.shape
    ops.conv2d_fwd(q.view(m, 1, 1, d), bankT, None, n_pad, 1, 1, 1, 0, out=out.view(m, 1, 1, n_pad))
    return out


def similarity_chunks(q, bankT, S=None, chunk_rows=None):
    """Yields ``(row0, S_chunk)``: the similarities of the rows [row0, row0 + len(S_chunk)) of ``q`` [m, d] to the bank, in
    chunks of ``chunk_rows`` rows (None: ``chunk_rows_of``, read at call time).  ``S_chunk`` is a view of one buffer that
    the next chunk overwrites: ``S`` (its rows are then the chunk size) or one made here.  Nothing for zero rows."""
    m, n_pad = q.shape[0], bankT.shape[1]
    if m == 0:
        return
    if S is None:
        S = torch.empty(min(chunk_rows or chunk_rows_of(n_pad), m), n_pad, device=q.device)
    chunk = S.shape[0]
    for i in range(0, m, chunk):
        r = min(chunk, m - i)
        yield i, similarities(q[i:i + r], bankT, S[:r])


# ---- images to features ----
def check_u8(x, what, who):
    """A device-resident image set: CUDA uint8 [n, H, W, 3], not empty."""
    if not torch.is_tensor(x) or not x.is_cuda or x.dtype != torch.uint8 or x.dim() != 4 or x.shape[3] != 3:
        raise RuntimeError('%s: the %s images must be a CUDA uint8 [n, H, W, 3] tensor' % (who, what))
    if x.shape[0] < 1:
        raise ValueError('%s: empty %s set' % (who, what))


def to_float_nchw(x_u8, idx, out):
    """out[i] = x_u8[idx[i]] as float NCHW in [0, 1] (ToTensor)."""
    out.copy_(x_u8.index_select(0, idx).permute(0, 3, 1, 2))
    return out.div_(255.0)


def extract_features(D, x_u8, batch, bankT=None):
    """Normalised penultimate features of the device-resident uint8 set ``x_u8`` [n, H, W, 3], ``batch`` images per
    forward.  Returns them as [n, d]; with ``bankT`` (``new_bank(n, d, device)``) writes column i of the bank per image
    instead and returns ``bankT``.  ``D`` must be in eval mode (the caller's business: this function touches no mode)."""
    if D.training:
        raise RuntimeError('features.extract_features: D must be in eval mode (train mode runs a power iteration per call)')
    check_u8(x_u8, 'given', 'features.extract_features')
    n, h, w, c = x_u8.shape
    dev = x_u8.device
    if batch < 1:
        raise ValueError('features.extract_features: batch must be at least 1, got %r' % (batch,))
    rows = None
    buf = torch.empty(min(batch, n), c, h, w, device=dev)
    with torch.no_grad():
        for i in range(0, n, batch):
            m = min(batch, n - i)
            x = to_float_nchw(x_u8, torch.arange(i, i + m, device=dev), buf[:m])
            z = normalize_rows(D.penultimate(x).reshape(m, -1))
            if bankT is not None:
                bankT[:, i:i + m].copy_(z.t())
                continue
            if rows is None:
                rows = torch.empty(n, z.shape[1], device=dev)
            rows[i:i + m].copy_(z)
    return bankT if bankT is not None else rows


# ---- checkpoints and sets ----
def load_frozen(module, path, device):
    """``module`` with the state dict of ``path``, on ``device``, frozen (evaluate/gan.py's ``freeze``)."""
    module.load_state_dict(torch.load(path, map_location='cpu'))
    return freeze(module.to(device))


def load_images(path, key, n=None):
    """uint8 [n, H, W, 3] images ``key`` of an npz, the first ``n`` of them."""
    with np.load(path) as z:
        if key not in z:
            raise ValueError('%s holds no %s' % (path, key))
        x = np.asarray(z[key])
    if x.dtype != np.uint8 or x.ndim != 4 or x.shape[3] != 3:
        raise ValueError('%s: %s must be uint8 [n, H, W, 3], got %s %s' % (path, key, x.dtype, x.shape))
    if n is not None:
        if n < 1:
            raise ValueError('%s: asked for %d images of %s' % (path, n, key))
        x = x[:n]
    if len(x) < 1:
        raise ValueError('%s: %s is empty' % (path, key))
    return np.ascontiguousarray(x)


def sample_u8(G, n, batch=500, seed=0):
    """``n`` images of ``G`` (in eval mode) at the fixed latents of ``seed`` as uint8 [n, H, W, 3] on G's device, quantised
    by ``ops.images_u8`` -- the kernel test_gan_sample.py writes ``samples.npz`` with, so fakes and reals pass through the
    same uint8 step.  The global random streams are left as they were (StyleGAN2's per-layer noise is drawn from a CUDA
    stream seeded with ``seed`` and restored)."""
    if G.training:
        raise RuntimeError('features.sample_u8: G must be in eval mode')
    if n < 1 or batch < 1:
        raise ValueError('features.sample_u8: n and batch must be at least 1, got %r, %r' % (n, batch))
    dev = next(G.parameters()).device
    out = None
    with torch.no_grad(), preserved_rng(dev):
        torch.cuda.manual_seed(int(seed))
        z = fixed_latent(G, n, seed)
        for i in range(0, n, batch):
            u8 = ops.images_u8(G(z[i:i + batch]).contiguous().float())
            if out is None:
                out = torch.empty((n,) + tuple(u8.shape[1:]), device=dev, dtype=torch.uint8)
            out[i:i + u8.shape[0]].copy_(u8)
    return out


def best_in_csv(path, column, upto_step, best):
    """The ``best`` (``min`` or ``max``) of ``column`` among the rows of a monitor's csv with step <= ``upto_step`` (None: no
    such row).  A resumed run passes the step of the checkpoint it starts from: a later row belongs to networks that were
    never saved (the row is written before the checkpoint) or that this run is about to supersede."""
    with open(path) as f:
        rows = [ln.split(',') for ln in f.read().split()[1:]]
    kept = [float(r[column]) for r in rows if int(r[0]) <= upto_step]
    return best(kept) if kept else None


# ---- the command line of "a real set against a fake set through a frozen encoder" (test_prdc.py, test_kid.py) ----
def real_fake_parser(description, seed_help, before_sizes=(), after_sizes=()):
    """The shared flags; ``before_sizes`` / ``after_sizes``: the evaluator's own ``(flag, keywords)`` pairs, listed before
    ``--n_real`` and after ``--n_fake``."""
    parser = ArgumentParser(description=description)
    parser.add_argument('model_path', type=str, help='Path to the (discriminator) checkpoint used as the encoder')
    parser.add_argument('architecture', type=str, help="The encoder's architecture")
    parser.add_argument('--real', required=True, type=str, help='npz with x_train uint8 [n, H, W, 3]')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--fake', default=None, type=str, help='npz with images uint8 [n, H, W, 3] (samples.npz of test_gan_sample.py)')
    src.add_argument('--gen', default=None, type=str, help='generator checkpoint to sample from at fixed latents of --seed')
    parser.add_argument('--gen_arch', default=None, type=str, help="with --gen: the generator's architecture (default: the encoder's)")
    for flag, keywords in before_sizes:
        parser.add_argument(flag, **keywords)
    parser.add_argument('--n_real', default=None, type=int, help='use the first N images of x_train (default: all)')
    parser.add_argument('--n_fake', default=None, type=int,
                        help='use the first N of --fake (default: all) / sample N from --gen (default: min(n_real, 10000))')
    for flag, keywords in after_sizes:
        parser.add_argument(flag, **keywords)
    parser.add_argument('--batch_size', default=500, type=int, help='images per forward (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help=seed_help)
    return parser


def real_fake_main(P, subject, check_sizes, evaluate, line, json_name):
    """The run behind such a command line ``P``.  Refusals in order: no GPU (``subject`` opens the sentence),
    ``--batch_size``, the sets' shapes, ``--n_fake``, then the evaluator's ``check_sizes(n_real, n_fake)`` -- all before the
    encoder is loaded.  ``evaluate(E, real_u8, fake_u8, seed)`` -> the result dict, printed as ``line(out)`` and written to
    ``json_name % seed`` next to the fakes.  Returns that path."""
    if not torch.cuda.is_available():
        raise RuntimeError('%s on the MI355X HIP path only (no CPU fallback)' % subject)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.batch_size < 1:
        raise ValueError('--batch_size must be at least 1, got %r' % (P.batch_size,))
    real = load_images(P.real, 'x_train', P.n_real)
    image_size = tuple(real.shape[1:])                                     # the image size comes from the data
    if P.fake:
        fake = load_images(P.fake, 'images', P.n_fake)
        if tuple(fake.shape[1:]) != image_size:
            raise ValueError('%s holds %s images, %s holds %s' % (P.real, image_size, P.fake, tuple(fake.shape[1:])))
        n_fake = len(fake)
    else:
        n_fake = min(len(real), 10000) if P.n_fake is None else P.n_fake
        if n_fake < 1:
            raise ValueError('--n_fake must be at least 1, got %r' % (n_fake,))
    check_sizes(len(real), n_fake)
    E = load_frozen(get_architecture(P.architecture, image_size)[1], P.model_path, dev)
    if P.fake:
        fake = torch.from_numpy(fake).to(dev)
    else:
        G = load_frozen(get_architecture(P.gen_arch or P.architecture, image_size)[0], P.gen, dev)
        fake = sample_u8(G, n_fake, P.batch_size, seed)
    with torch.no_grad():
        out = evaluate(E, torch.from_numpy(real).to(dev), fake, seed)
    print(line(out), flush=True)
    path = os.path.join(Path(P.fake or P.gen).parent, json_name % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    return path
