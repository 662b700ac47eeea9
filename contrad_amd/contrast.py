"""Label-free diagnostics of the contrastive side of a discriminator on held-out views: the rank of the positive (the
contrastive accuracy), alignment and uniformity (Wang & Isola 2020) and the NT-Xent value itself.  An ADDITION of this
project: the reference logs the value of the loss and nothing else about it.  The three numbers,
taken under the run's own ``--aug``, are what the augmentation strength is read against: they tell "the NT-Xent value
went down" from "the representation collapsed".

    python test_contrast.py <run>/dis.pt sndcgan --data celeba.npz --aug simclr --temp 0.1
    python test_contrast.py <run>/dis.pt sndcgan --synthetic --n 2000 --batch_size 512 --t 2

Views and rows.  ``A = aug(x)`` and ``B = aug(x)`` are two independent draws on the first ``n`` images of a device-resident
uint8 set; ``aug.sample()`` runs under ``preserved_rng`` with the host generators seeded with the evaluation seed, so the
same views come back at every evaluation and the global streams are untouched.  D runs in eval mode under ``no_grad``:
``D(x, projection=True, penultimate=True)``.  ``p_A``, ``p_B`` are the L2-normalised projection rows, ``f_A``, ``f_B`` the
L2-normalised penultimate rows.  Every quantity is reported for the projection space; alignment and uniformity also for the
penultimate space (keys ``align_pen``, ``uniform_pen``).

  * alignment: with u(a, b) = max(2 - 2 a.b, 0), ``align = mean_i u(A_i, B_i)`` (the reference's alpha = 2), in float64 from
    ``ops.dot_sums(A, B)``: the kernel returns the sum of the n row dots, so the clamp is taken on the mean,
    max(2 - 2 sum / n, 0); a single row lies below 0 by no more than the rounding of its two fp32 normalisations;
  * uniformity: ``uniform = log((1 / (n (n - 1))) sum_{i != j} exp(-t u(A_i, A_j)))``, t = 2 by default, over view A alone
    and over all n rows (not per block); the self pair is left out by index (``ops.gauss_sums``, csrc/kid.hip kind 3, on
    the row chunks of contrad_amd/features.py);
  * NT-Xent: the rows are cut into blocks of ``batch`` images (default: the run's training batch, so value and chance level
    are those of the training loss); a block is the 2b rows [A_blk | B_blk]; ``nt_xent`` is ``ops.contrast_fwd`` at the run's
    ``--temp``, averaged over blocks weighted by rows.  A last block of fewer than 2 images is refused;
  * positive rank: for row i of a block, ``rank_i`` = #{j not in {i, pos(i)} : s_ij >= s_i,pos(i)}.  Ties count against the
    positive; the row itself is left out by index, never by value.  ``acc@1 = mean[rank = 0]``, ``acc@5 = mean[rank < 5]``,
    ``rank_mean`` the mean rank, all over the 2n rows, as fractions; the chance level 1 / (2b - 2) is reported.
    Counting: the block's S = Z Z^T gets a NaN diagonal (a NaN hits nothing), the threshold of column j is read from the
    same column of the same matrix (S[pos(j)][j]: nothing relies on the fp32 GEMM being bitwise symmetric), one
    ``ops.prdc_count`` pass counts exactly in integers, and the positive's own hit is subtracted.

The device is read once, at the end.  ``--contrast_data`` of the training scripts runs this at every ``--evaluate_every``
through ``ContrastMonitor`` (evaluate/gan.py's ``WeightsMonitor``: a discriminator of its own, so that the training
trajectory does not move by a bit).
"""
import inspect
import json
import math
import os
from argparse import ArgumentParser
from pathlib import Path

import numpy as np
import torch

from . import config, features, ops
from .evaluate.gan import WeightsMonitor, load_x_train, own_network, preserved_rng
from .hooks import Hook

KEYS = ('nt_xent', 'acc@1', 'acc@5', 'rank_mean', 'align', 'uniform', 'align_pen', 'uniform_pen')
CSV_HEADER = 'step,' + ','.join(KEYS)
MODE_NT_XENT = 0                                                    # contrad_contrast_fwd's mode (training/criterion.py)


def chance_level(batch):
    """1 / (2b - 2): the probability that the positive is first among the 2b - 2 other rows of a block."""
    return 1.0 / (2 * int(batch) - 2)


def check_sizes(n, batch, temp, t):
    """The host refusals, before any GPU work -> the block size min(batch, n)."""
    if int(n) < 2:
        raise ValueError('contrast: n = %r: a positive needs a competitor, at least 2 images' % (n,))
    if int(batch) < 2:
        raise ValueError('contrast: batch = %r: a block of fewer than 2 images has no negatives' % (batch,))
    if not float(temp) > 0 or not math.isfinite(float(temp)):
        raise ValueError('contrast: temp must be positive and finite, got %r' % (temp,))
    if not (math.isfinite(float(t)) and float(t) >= 0):
        raise ValueError('contrast: t must be finite and not negative, got %r' % (t,))
    b = min(int(batch), int(n))
    if int(n) % b == 1:
        raise ValueError('contrast: %d images in blocks of %d leave a last block of 1 image: no negatives there' % (n, b))
    return b


def _check_rows(mats):
    shapes = [tuple(m.shape) if torch.is_tensor(m) else None for m in mats]
    if None in shapes or any(len(s) != 2 for s in shapes):
        raise ValueError('contrast: the views are (n, d) matrices, got %s' % (shapes,))
    if shapes[0] != shapes[1]:
        raise ValueError('contrast: the two views differ in shape: %s and %s' % (shapes[0], shapes[1]))
    return shapes[0]


def _align_uniform(A, B, t, cells):
    """cells[0] = sum_i A_i . B_i, cells[1] = sum_{i != j} exp(-t u(A_i, A_j)) (float64, on the device)."""
    n, d = A.shape
    ops.dot_sums(A, B, d, out=cells[0:1])
    for i, Sc in features.similarity_chunks(A, features.bank_of(A)):
        ops.gauss_sums(Sc, n, t, self0=i, out=cells[1:2], accumulate=i > 0)


def _align(dots, n):
    """max(2 - 2 mean dot, 0); a NaN stays a NaN."""
    return max(2.0 - 2.0 * dots / n, 0.0) if dots == dots else float('nan')


def _uniform(total, n):
    """log of the mean over the n (n - 1) ordered pairs; a NaN stays a NaN, a sum that underflowed to 0 gives -inf."""
    if total != total:
        return float('nan')
    return math.log(total / (float(n) * (n - 1))) if total > 0 else float('-inf')


def block_ranks(z, b):
    """rank (2b,) int64 of the rows of one block z = [A_blk | B_blk] (2b, d) of unit rows, on the device."""
    R = 2 * b
    bank = features.bank_of(z)
    S = torch.empty(R, bank.shape[1], device=z.device)
    for _, _ in features.similarity_chunks(z, bank, S=S):
        pass
    S[:, :R].fill_diagonal_(float('nan'))                               # the row itself: left out by index
    cols = torch.arange(R, device=z.device)
    thr = S[(cols + b) % R, cols].contiguous()                          # S[pos(j)][j]: the same column of the same matrix
    hits = torch.zeros(R, device=z.device, dtype=torch.int32)
    ops.prdc_count(S, R, thr_col=thr, col_hits_c=hits)
    return hits.long() - 1                                              # the positive's own hit


def _block(z, b, temp, cells):
    """One block z = [A_blk | B_blk] (2b, d): cells += (2b * nt_xent, #[rank = 0], #[rank < 5], sum of ranks)."""
    loss, _ = ops.contrast_fwd(z, b, MODE_NT_XENT, temp)
    rank = block_ranks(z, b)
    cells += torch.stack([loss[0].double() * (2 * b), (rank == 0).sum().double(), (rank < 5).sum().double(), rank.sum().double()])


def contrast_stats(pA, pB, batch, temp, t=2.0, normalize=True, fA=None, fB=None):
    """The diagnostics of given feature rows: ``pA``, ``pB`` CUDA fp32 (n, d) projection rows of the two views (d <= 256, the
    NT-Xent kernel's limit), ``fA``, ``fB`` the penultimate rows (optional: ``align_pen`` / ``uniform_pen``).  ``normalize``:
    L2-normalise the rows here (False: the caller did).  Returns a dict of floats: ``KEYS`` (the ``_pen`` ones with ``fA``),
    ``chance``, ``n``, ``batch`` (the block size, min(batch, n)), ``temp``, ``t``."""
    n, d = _check_rows((pA, pB))
    if (fA is None) != (fB is None):
        raise ValueError('contrast: the penultimate rows come as a pair')
    if fA is not None and _check_rows((fA, fB))[0] != n:
        raise ValueError('contrast: %d penultimate rows for %d projection rows' % (fA.shape[0], n))
    b = check_sizes(n, batch, temp, t)
    for m in (pA, pB, fA, fB):
        if m is not None and (not m.is_cuda or m.dtype != torch.float32):
            raise RuntimeError('contrast: the rows must be CUDA float32 matrices (the MI355X HIP path only, no CPU fallback)')
    prep = features.normalize_rows if normalize else (lambda m: m.contiguous())
    pA, pB = prep(pA), prep(pB)
    cells = torch.zeros(8, device=pA.device, dtype=torch.float64)
    _align_uniform(pA, pB, t, cells[0:2])
    if fA is not None:
        _align_uniform(prep(fA), prep(fB), t, cells[2:4])
    for i in range(0, n, b):
        _block(torch.cat([pA[i:i + b], pB[i:i + b]]), min(b, n - i), temp, cells[4:8])
    c = cells.cpu().tolist()                                            # the one device-to-host read
    out = {'nt_xent': c[4] / (2 * n), 'acc@1': c[5] / (2 * n), 'acc@5': c[6] / (2 * n), 'rank_mean': c[7] / (2 * n),
           'align': _align(c[0], n), 'uniform': _uniform(c[1], n)}
    if fA is not None:
        out['align_pen'], out['uniform_pen'] = _align(c[2], n), _uniform(c[3], n)
    out.update({'chance': chance_level(b), 'n': n, 'batch': b, 'temp': float(temp), 't': float(t)})
    return out


# ---- from images ----
def one_view(aug, x):
    """One draw of ``aug`` on the float NCHW batch ``x``: ``sample()`` on the host (the global generators), ``apply()`` on the
    device.  A module without ``sample`` (``--aug none``) is the identity."""
    if not hasattr(aug, 'sample'):
        return x
    B, _, d2, d3 = x.shape
    sized = len(inspect.signature(aug.sample).parameters) == 3           # the SimCLR pipelines and diffaug; hflip / hfrt take B alone
    drawn = aug.sample(B, d2, d3) if sized else aug.sample(B)
    return aug.apply(x, *drawn) if isinstance(drawn, tuple) else aug.apply(x, drawn)


def contrast_of(D, x_u8, aug, n, batch, temp, t=2.0, seed=0, fwd_batch=500):
    """The diagnostics of the first ``n`` images of the device-resident uint8 set ``x_u8`` [N, H, W, 3] under ``aug`` (the
    module ``get_augment`` returns).  ``D``: on the GPU, in eval mode.  ``seed`` seeds the host generators that ``sample()``
    reads, inside ``preserved_rng``.  ``fwd_batch``: images per forward."""
    features.check_u8(x_u8, 'given', 'contrast.contrast_of')
    check_sizes(n, batch, temp, t)
    if n > x_u8.shape[0]:
        raise ValueError('contrast.contrast_of: asked for %d images of a set of %d' % (n, x_u8.shape[0]))
    if fwd_batch < 1:
        raise ValueError('contrast.contrast_of: fwd_batch must be at least 1, got %r' % (fwd_batch,))
    if D.training:
        raise RuntimeError('contrast.contrast_of: D must be in eval mode (train mode runs a power iteration per call)')
    dev = x_u8.device
    _, h, w, c = x_u8.shape
    rows = {}
    buf = torch.empty(min(fwd_batch, n), c, h, w, device=dev)
    with torch.no_grad(), preserved_rng(dev):
        torch.default_generator.manual_seed(int(seed))                  # (the CPU generator alone: sample() draws on the host)
        np.random.seed(int(seed) % (1 << 32))
        for i in range(0, n, fwd_batch):
            m = min(fwd_batch, n - i)
            x = features.to_float_nchw(x_u8, torch.arange(i, i + m, device=dev), buf[:m])
            for view in 'AB':
                _, aux = D(one_view(aug, x), projection=True, penultimate=True)
                for key, name in (('p', 'projection'), ('f', 'penultimate')):
                    z = features.normalize_rows(aux[name].reshape(m, -1))
                    if key + view not in rows:
                        rows[key + view] = torch.empty(n, z.shape[1], device=dev)
                    rows[key + view][i:i + m].copy_(z)
        return contrast_stats(rows['pA'], rows['pB'], batch, temp, t, normalize=False, fA=rows['fA'], fB=rows['fB'])


def csv_row(step, out):
    return '%d,' % step + ','.join('%.6f' % out[k] for k in KEYS)


def log_line(step, out):
    return ('[Steps %7d] [NT-Xent %.4f] [pos Acc@1 %.4f Acc@5 %.4f, chance %.4f] [rank %.2f] [align %.4f] [uniform %.4f]'
            % (step, out['nt_xent'], out['acc@1'], out['acc@5'], out['chance'], out['rank_mean'], out['align'], out['uniform']))


class ContrastMonitor(WeightsMonitor):
    """``--contrast_data`` on rank 0: the diagnostics of the training discriminator's weights at every evaluation, appended
    as ``step,nt_xent,acc@1,acc@5,rank_mean,align,uniform,align_pen,uniform_pen`` to ``contrast_<eval_seed>.csv``
    (evaluate/gan.py's ``WeightsMonitor``).  The views are drawn from host generators seeded with the evaluation seed.
    ``aug`` / ``temp`` default to the run's (``P.augment_fn``, ``P.temp``); ``batch`` is the run's training batch."""

    def __init__(self, logdir, architecture, image_size, device, seed, data_path, n=2000, t=2.0, P=None, aug=None, batch=None,
                 temp=None, fwd_batch=500):
        self.aug = aug if aug is not None else P.augment_fn
        self.temp = float(P.temp if temp is None else temp)
        if batch is None:
            raise ValueError('contrast: the monitor needs the block size (the training batch)')
        x = load_x_train(data_path, image_size, 'discriminator takes')
        self.n, self.t, self.fwd_batch = min(int(n), len(x)), float(t), fwd_batch
        self.batch = check_sizes(self.n, batch, self.temp, self.t)
        self.x = torch.from_numpy(x[:self.n]).to(device)                   # the uint8 set goes to the device once
        super().__init__(logdir, device, seed, own_network('D', architecture, image_size, device, P),
                         [('contrast_%d.csv', CSV_HEADER, csv_row)], which='D')

    def evaluate(self):
        return contrast_of(self.D, self.x, self.aug, self.n, self.batch, self.temp, self.t, self.eval_seed, self.fwd_batch)


# ---- the training scripts' hook ----
def _refusals(H, P):
    if H.contrast_data:
        if H.contrast_n < 2:
            raise ValueError('--contrast_n must be at least 2, got %r' % (H.contrast_n,))
        if not (math.isfinite(H.contrast_t) and H.contrast_t >= 0):
            raise ValueError('--contrast_t must be finite and not negative, got %r' % (H.contrast_t,))


HOOK = Hook(
    flags=(('contrast_data', None, dict(type=str, help='npz with x_train uint8 [n, H, W, 3] (no labels needed): rank 0 appends the NT-Xent value, the rank '
                                                       'of the positive (Acc@1, Acc@5, mean rank), alignment and uniformity of D on two held-out views '
                                                       'under the run\'s --aug and --temp to contrast_<seed>.csv at every evaluate_every; the training '
                                                       'trajectory is unchanged')),
           ('contrast_n', 2000, dict(type=int, help='with --contrast_data: the first N images of x_train (default: 2000)')),
           ('contrast_t', 2.0, dict(type=float, help='with --contrast_data: t of the uniformity potential exp(-t |a - b|^2) (default: 2)'))),
    switch='contrast_data', shown='D', refusals=_refusals,
    # blocks of the training batch (all ranks' images)
    build=lambda H, run: ContrastMonitor(*run.head, H.contrast_data, n=H.contrast_n, t=H.contrast_t, P=run.P, batch=run.batch),
    log_lines=lambda monitor, step, out: [log_line(step, out)])
add_hook_arguments, check_hook_arguments = HOOK.add_arguments, HOOK.check


# ---- the command line ----
def parse_args(argv=None):
    parser = ArgumentParser(description='Testing script: contrastive diagnostics of a discriminator on held-out views (one process, one GPU)')
    parser.add_argument('model_path', type=str, help='Path to the (discriminator) model checkpoint')
    parser.add_argument('architecture', type=str, help='Architecture')
    parser.add_argument('--data', default=None, type=str, help='npz with x_train uint8 [n, H, W, 3] (labels are not read)')
    parser.add_argument('--synthetic', action='store_true', help='seeded synthetic set instead of a dataset')
    parser.add_argument('--synthetic_image', default=32, type=int, help='side of the synthetic images (default: 32)')
    parser.add_argument('--aug', default='simclr', type=str, help="the augmentation of the views, as the run's --aug (default: simclr)")
    parser.add_argument('--temp', default=0.1, type=float, help="NT-Xent temperature, as the run's --temp (default: 0.1)")
    parser.add_argument('--n', default=2000, type=int, help='use the first N images (default: 2000; clamped to the set)')
    parser.add_argument('--batch_size', default=None, type=int,
                        help="images per NT-Xent block (default: the batch_size of the *.gin beside the checkpoint, 64 without one)")
    parser.add_argument('--t', default=2.0, type=float, help='t of the uniformity potential (default: 2)')
    parser.add_argument('--fwd_batch', default=500, type=int, help='images per forward (default: 500)')
    parser.add_argument('--seed', default=None, type=int, help='file-name tag and seed of the views and of --synthetic (default: drawn)')
    return parser.parse_args(argv)


def bind_augment_config(logdir):
    """The augmentation's gin bindings: the defaults, then the first ``*.gin`` beside the checkpoint when there is one (as
    sample.py finds the run's configuration).  Returns the run's ``options`` bindings ({} without a run file)."""
    gins = sorted(Path(logdir).glob('*.gin'))
    config.clear_config()
    files = [os.path.join(config.CONFIG_ROOT, 'defaults', 'augment.gin')]
    if gins:
        files = [os.path.join(config.CONFIG_ROOT, 'defaults', 'gan.gin')] + files + [str(gins[0])]
    config.parse_config_files_and_bindings(files)
    return dict(config.get_bindings('options') or {}) if gins else {}


def main(argv=None):
    from .augment import get_augment
    from .lineval import synthetic_set
    from .models.gan import get_architecture
    P = parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError('the contrastive diagnostics run on the MI355X HIP path only (no CPU fallback)')
    seed = int(np.random.randint(10000)) if P.seed is None else P.seed
    if P.n < 2:
        raise ValueError('--n must be at least 2, got %r' % (P.n,))
    if P.synthetic:
        x = synthetic_set(seed, 10, P.n, 1, size=P.synthetic_image)['x_train']
    elif P.data:
        x = features.load_images(P.data, 'x_train', P.n)
    else:
        raise RuntimeError('no dataset reader is installed here: pass --data FILE.npz (x_train) or --synthetic')
    logdir = Path(P.model_path).parent
    options = bind_augment_config(logdir)
    n = len(x)
    batch = check_sizes(n, P.batch_size if P.batch_size is not None else int(options.get('batch_size', 64)), P.temp, P.t)
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    image_size = tuple(x.shape[1:])                                        # the image size comes from the data
    aug = get_augment(mode=P.aug).to(dev)
    D = features.load_frozen(get_architecture(P.architecture, image_size)[1], P.model_path, dev)
    out = contrast_of(D, torch.from_numpy(x).to(dev), aug, n, batch, P.temp, P.t, seed, P.fwd_batch)
    out.update({'aug': P.aug, 'seed': seed})
    print(log_line(0, out).split('] ', 1)[1] + ' on %d images in blocks of %d (aug %s, T %g, t %g)' % (n, batch, P.aug, P.temp, P.t), flush=True)
    path = os.path.join(logdir, 'contrast_%d.json' % seed)
    with open(path, 'w') as f:
        json.dump(out, f)
    return path


if __name__ == '__main__':
    main()
