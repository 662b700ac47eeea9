"""Sample quality without an Inception network: improved precision / recall (Kynkaanniemi et al. 2019) and density /
coverage (Naeem et al. 2020) of generated images in the feature space of a FROZEN discriminator (a ContraD or
``--mode=simclr_only`` checkpoint: a self-supervised encoder, as Morozov et al. 2021 evaluate with).  An ADDITION of this
project: the reference tracks FID, which is out of scope here (DESIGN.md sections 8 and 16).  The numbers are comparable
between checkpoints and runs evaluated with the same encoder file, not with Inception-based numbers of papers.

    python test_prdc.py enc/dis.pt sndcgan --real cifar10.npz --fake <run>/samples_7_n10000/samples.npz
    python test_prdc.py enc/dis.pt sndcgan --real cifar10.npz --gen <run>/gen.pt --n_fake 10000 --seed 7

The definitions live in SIMILARITY space.  Features are ``D.penultimate`` in eval mode with L2-normalised rows
(``features.extract_features``); on the unit sphere ||a - b||^2 = 2 - 2 a.b, so "inside the k-NN ball" is "similarity >= a
threshold" and every comparison is made on the fp32 similarities the conv engine writes: no squared distance is formed,
nothing cancels.  (The papers use raw Euclidean distances of unnormalised features.)  With R the n_r real rows, F the n_f
fake rows, S_XY = X Y^T:

    t_R[i] = k-th largest of S_RR[i][j], j != i        t_F[j] = k-th largest of S_FF[j][l], l != j     (self left out by index)
    hit_c[j][i] = S_FR[j][i] >= t_R[i]                 hit_r[j][i] = S_FR[j][i] >= t_F[j]              (inclusive; NaN: no hit)
    precision = mean_j any_i hit_c     density = sum_j sum_i hit_c / (k n_f)     coverage = mean_i any_j hit_c
    recall = mean_i any_j hit_r

  * banks and the row chunks of S: contrad_amd/features.py;
  * csrc/prdc.hip: ``prdc_kth`` per chunk of S_RR and S_FF (``self0`` = the chunk's first row), ``prdc_count`` per chunk of S_FR;
  * the four metrics are ratios of integers counted on the device; the host reads them once and divides in float64.

``--prdc_data`` / ``--prdc_encoder`` of the training scripts run this at every ``--evaluate_every`` through ``PRDCMonitor``
(evaluate/gan.py's ``WeightsMonitor``: modules of its own, so that the training trajectory does not move by a bit).  ``--prdc_best
METRIC`` keeps ``gen_best.pt`` / ``dis_best.pt`` (/ ``gen_ema_best.pt``), the names the reference gives its best-FID
checkpoints, for the best value of that metric.  ``--prdc_kid`` adds the kernel distance of contrad_amd/kid.py to every
evaluation (``kid_<seed>.csv``; ``--prdc_best kid`` selects its minimum); ``--prdc_kid_kernel rq`` makes that the
rational-quadratic distance, in ``kid_rq_<seed>.csv``.  ``--prdc_fd`` adds the Frechet distance of contrad_amd/fd.py
(``fd_<seed>.csv``; it records only).
"""
import torch

from . import fd as fd_mod
from . import features, ops
from . import kid as kid_mod
from . import nearest
from .evaluate.gan import WeightsMonitor, frozen_encoder, load_x_train, own_network, preserved_rng
from .hooks import Hook

METRICS = ('precision', 'recall', 'density', 'coverage')
CSV_HEAD = 'step,' + ','.join(METRICS)
BEST_CHOICES = METRICS + ('kid',)                                           # --prdc_best: kid (contrad_amd/kid.py) is minimised


def _tracked(metric):
    """Where ``PRDCMonitor`` finds a ``--prdc_best`` metric: (which of its csv files, the column, +1 maximised / -1 minimised)."""
    return (1, 1, -1) if metric == 'kid' else (0, 1 + METRICS.index(metric), 1)


def _rows(feats, what, normalize):
    if not torch.is_tensor(feats) or not feats.is_cuda or feats.dtype != torch.float32 or feats.dim() != 2:
        raise RuntimeError('prdc: the %s features must be a CUDA float32 (n, d) matrix' % what)
    if feats.shape[0] < 1:
        raise ValueError('prdc: empty %s set' % what)
    return features.normalize_rows(feats) if normalize else feats.contiguous()


def check_k(k, n_real, n_fake):
    if int(k) < 1:
        raise ValueError('prdc: k must be at least 1, got %r' % (k,))
    if int(k) >= min(n_real, n_fake):
        raise ValueError('prdc: k = %d needs more than k images in both sets (%d real, %d fake): a row has n - 1 neighbours'
                         % (k, n_real, n_fake))


def kth_similarity(rows, bankT, k):
    """t[i]: the k-th largest similarity of row i of ``rows`` [n, d] to the OTHER columns of its own bank."""
    n = rows.shape[0]
    thr = torch.empty(n, device=rows.device)
    for i, S in features.similarity_chunks(rows, bankT):
        ops.prdc_kth(S, n, k, self0=i, out=thr[i:i + S.shape[0]])
    return thr


def real_state_of(real_feats, k, normalize=True):
    """``(bankT, t_R)`` of a real set: what ``prdc`` needs of it, for a caller whose real set does not change."""
    rows = _rows(real_feats, 'real', normalize)
    check_k(k, rows.shape[0], rows.shape[0])
    bankT = features.bank_of(rows)
    return bankT, kth_similarity(rows, bankT, int(k))


def prdc(real_feats, fake_feats, k=5, real_state=None, normalize=True):
    """The four metrics of fake feature rows [n_f, d] against real ones [n_r, d] (CUDA fp32).  ``normalize``: L2-normalise the
    rows here (False: the caller did, as ``extract_features`` does).  ``real_state``: ``real_state_of`` of the same real set
    and k (``real_feats`` is then not read and may be None).  Returns precision, recall, density, coverage, the integer
    counts behind them and n_real, n_fake, k."""
    k = int(k)
    fake = _rows(fake_feats, 'fake', normalize)
    if real_state is None:
        real = _rows(real_feats, 'real', normalize)
        check_k(k, real.shape[0], fake.shape[0])                           # (before the real set's GEMMs)
        bankT = features.bank_of(real)
        real_state = (bankT, kth_similarity(real, bankT, k))
    bankT, t_R = real_state
    n_r, n_f, dev = t_R.numel(), fake.shape[0], fake.device
    check_k(k, n_r, n_f)
    if bankT.shape[0] != fake.shape[1] or bankT.shape[1] != ops.round_up(n_r, 4):
        raise RuntimeError('prdc: a real bank of %s for %d thresholds and fake features of width %d'
                           % (tuple(bankT.shape), n_r, fake.shape[1]))
    t_F = kth_similarity(fake, features.bank_of(fake), k)
    row_hits = torch.empty(n_f, device=dev, dtype=torch.int32)
    col_c = torch.zeros(n_r, device=dev, dtype=torch.int32)
    col_r = torch.zeros(n_r, device=dev, dtype=torch.int32)
    for i, S in features.similarity_chunks(fake, bankT):
        m = S.shape[0]
        ops.prdc_count(S, n_r, thr_row=t_F[i:i + m], thr_col=t_R, row_hits=row_hits[i:i + m], col_hits_c=col_c, col_hits_r=col_r)
    counts = torch.stack([(row_hits > 0).sum(), row_hits.sum(dtype=torch.int64), (col_c > 0).sum(), (col_r > 0).sum()])
    n_prec, n_hits, n_cov, n_rec = (int(v) for v in counts.tolist())           # the one device-to-host read
    return {'precision': n_prec / n_f, 'recall': n_rec / n_r, 'density': n_hits / (k * n_f), 'coverage': n_cov / n_r,
            'fakes_in_real_balls': n_prec, 'hits': n_hits, 'reals_with_a_fake': n_cov, 'reals_in_fake_balls': n_rec,
            'n_real': n_r, 'n_fake': n_f, 'k': k}


def real_state_of_images(encoder, real_u8, k, batch=500):
    features.check_u8(real_u8, 'real', 'prdc')
    return real_state_of(features.extract_features(encoder, real_u8, batch), k, normalize=False)


def prdc_of(encoder, real_u8, fake_u8, k=5, batch=500, real_state=None):
    """``prdc`` of device-resident uint8 [n, H, W, 3] sets through ``encoder`` (on the GPU, in eval mode), ``batch`` images
    per trunk forward.  ``real_state``: ``real_state_of_images`` of the real set (``real_u8`` is then not read)."""
    features.check_u8(fake_u8, 'fake', 'prdc')
    if real_state is None:
        features.check_u8(real_u8, 'real', 'prdc')
        if tuple(real_u8.shape[1:]) != tuple(fake_u8.shape[1:]):
            raise ValueError('prdc: the real images are %s, the fake ones %s' % (tuple(real_u8.shape[1:]), tuple(fake_u8.shape[1:])))
        check_k(k, real_u8.shape[0], fake_u8.shape[0])
        real_state = real_state_of_images(encoder, real_u8, k, batch)
    return prdc(None, features.extract_features(encoder, fake_u8, batch), k, real_state=real_state, normalize=False)


def best_in_csv(path, metric, upto_step):
    """The largest ``metric`` among the rows of a ``prdc_<seed>.csv`` with step <= ``upto_step`` (None: no such row)."""
    return features.best_in_csv(path, 1 + METRICS.index(metric), upto_step, max)


def csv_line(step, out):
    return '%d,%s' % (step, ','.join('%.6f' % out[m] for m in METRICS))


class PRDCMonitor(WeightsMonitor):
    """``--prdc_data`` on rank 0: precision / recall / density / coverage of the training generator's weights at every
    evaluation, appended as ``step,precision,recall,density,coverage`` to ``prdc_<eval_seed>.csv`` (evaluate/gan.py's
    ``WeightsMonitor``).  It owns its encoder (``encoder_path``, loaded once and frozen: the yardstick must not move with the
    run); the fakes come from fixed latents of the eval seed.  The real features and t_R are computed once, here.
    ``best``: one of BEST_CHOICES; ``update`` then says whether the evaluation improved it (the caller writes the
    ``*_best.pt`` files); a run resumed from the checkpoint of step ``resumed_step`` reads the best value up to that step
    back from its csv (``features.best_in_csv``).  ``kid`` (``--prdc_kid``): each evaluation also appends ``step,kid,kid_std``
    to ``kid_<eval_seed>.csv`` (contrad_amd/kid.py); ``best`` may then be ``'kid'``, which is minimised.  ``kid_kernel``
    (``--prdc_kid_kernel``): 'rq' computes the rational-quadratic distance instead, into ``kid_rq_<eval_seed>.csv`` (never into
    ``kid_<eval_seed>.csv``: the two are different numbers), which ``best='kid'`` then tracks and reads back.  ``auth``
    (``--prdc_auth``): the real features are extracted once for both states -- ``real_state_of`` and ``nearest.real_state_of``
    on the same bank -- and each evaluation also appends ``step,authenticity,nearest_mean`` to ``auth_<eval_seed>.csv``
    (contrad_amd/nearest.py: the memorisation check); it records only and is no ``best``.  ``fd`` (``--prdc_fd``): the real
    state of contrad_amd/fd.py is made once from the same bank and each evaluation also appends
    ``step,fd,mean_term,trace_fake,cross_term,tail`` to ``fd_<eval_seed>.csv``, the Frechet distance of the same fake
    features after ``fd_iter`` Newton-Schulz steps (``--prdc_fd_iter``); it records only and is no ``best``."""

    def __init__(self, logdir, architecture, image_size, device, seed, data_path, encoder_path, encoder_arch=None, k=5,
                 n_fake=10000, batch=500, best=None, resumed_step=0, P=None, kid=False, kid_kernel='poly3', auth=False, fd=False,
                 fd_iter=fd_mod.N_ITER):
        real = load_x_train(data_path, image_size, 'generator makes')
        check_k(k, len(real), n_fake)
        if best is not None and best not in BEST_CHOICES:
            raise ValueError('--prdc_best %r (one of %s)' % (best, ', '.join(BEST_CHOICES)))
        if best == 'kid' and not kid:
            raise ValueError('--prdc_best kid needs --prdc_kid')
        kid_mod.check_kernel_name(kid_kernel)
        if kid_kernel != 'poly3' and not kid:
            raise ValueError('--prdc_kid_kernel needs --prdc_kid')
        if kid:
            kid_mod.check_sizes(len(real), n_fake)
        if auth and len(real) < 2:
            raise ValueError('--prdc_auth needs at least 2 real images (%d)' % len(real))
        if fd:
            fd_mod.check_sizes(len(real), n_fake, fd_iter)
        self.k, self.n_fake, self.batch, self.metric = int(k), int(n_fake), int(batch), best
        self.kid_kernel = kid_kernel if kid else None
        self.auth_state = self.fd_state = None
        self.fd_iter, self.n_real = int(fd_iter), len(real)
        G = own_network('G', architecture, image_size, device, P)
        self.E = frozen_encoder(encoder_arch or architecture, image_size, encoder_path, device)
        with torch.no_grad(), preserved_rng(device):
            if not auth:
                self.real_state = real_state_of_images(self.E, torch.from_numpy(real).to(device), self.k, self.batch)
            else:                                                          # one extraction, one bank, both states
                real_u8 = torch.from_numpy(real).to(device)
                features.check_u8(real_u8, 'real', 'prdc')
                feats = features.extract_features(self.E, real_u8, self.batch)
                self.real_state = real_state_of(feats, self.k, normalize=False)
                self.auth_state = nearest.real_state_of(feats, normalize=False, bankT=self.real_state[0])
            if fd:                                                         # the same bank: centred once, here
                self.fd_state = fd_mod.real_state_of(self.real_state[0], self.n_real)
        super().__init__(logdir, device, seed, G,
                         [('prdc_%d.csv', CSV_HEAD, csv_line)] + ([(kid_csv_name(kid_kernel), kid_mod.CSV_HEAD, kid_mod.csv_line)] if kid else []) +
                         ([('auth_%d.csv', nearest.CSV_HEAD, nearest.csv_line)] if auth else []) +
                         ([('fd_%d.csv', fd_mod.CSV_HEAD, fd_mod.csv_line)] if fd else []),     # (after the files --prdc_best tracks)
                         which='G')
        self.best = None
        if best is not None:                                               # (a file made just now holds no row: None)
            j, column, sign = _tracked(best)
            self.best = features.best_in_csv(self.files[j][0], column, resumed_step, min if sign < 0 else max)

    def evaluate(self):
        fake = features.sample_u8(self.G, self.n_fake, self.batch, self.eval_seed)
        features.check_u8(fake, 'fake', 'prdc')
        feats = features.extract_features(self.E, fake, self.batch)
        out = prdc(None, feats, self.k, real_state=self.real_state, normalize=False)
        if self.kid_kernel is not None:                                    # the same fake features, the same real rows (bankT)
            d = kid_mod.kid(None, feats, seed=self.eval_seed, normalize=False, real_bank=(self.real_state[0], self.n_real),
                            kernel=self.kid_kernel)
            out['kid'], out['kid_std'] = d['kid'], d['kid_std']
        if self.auth_state is not None:                                    # the same fake features, the same real bank
            a = nearest.authenticity(None, feats, real_state=self.auth_state, normalize=False)
            out['authenticity'], out['nearest_mean'], out['real_nearest_mean'] = a['authenticity'], a['nearest_mean'], a['real_nearest_mean']
        if self.fd_state is not None:                                      # the same fake features, the real state made once
            f = fd_mod.fd(None, feats, self.fd_iter, normalize=False, real_state=self.fd_state)
            out['fd'] = f['fd']
            for name in ('mean_term', 'trace_fake', 'cross_term', 'tail'):
                out['fd_' + name] = f[name]
        return out

    def update(self, step, generator):
        """One evaluation of ``generator``'s weights (G, or g_ema in the StyleGAN2 loops) -> the metrics, with
        ``improved``: the tracked metric rose above (kid: fell below) the best so far (False without ``best``; a tie keeps
        the earlier).  With ``kid`` the kernel distance of the same fake features (contrad_amd/kid.py: the subsets of the
        eval seed, the same at every evaluation) comes as ``kid`` / ``kid_std`` and goes to ``kid_<eval_seed>.csv``."""
        out = super().update(step, generator)
        out['improved'] = False
        if self.metric is not None:
            j, column, sign = _tracked(self.metric)
            value = float(self.lines[j].split(',')[column])                # as the csv keeps it: a resumed run compares alike
            if self.best is None or sign * value > sign * self.best:
                self.best, out['improved'] = value, True
        return out

    def log_lines(self, step, out):
        """The lines of the training log for ``out`` of ``update``: ``[best ...]`` closes the line of the tracked metric."""
        mark = lambda here: ' [best %s]' % self.metric if out['improved'] and here else ''
        lines = ['[Steps %7d] [precision %.4f] [recall %.4f] [density %.4f] [coverage %.4f]%s' % (
            step, out['precision'], out['recall'], out['density'], out['coverage'], mark(self.metric != 'kid'))]
        if 'kid' in out:
            lines.append('[Steps %7d] [%s %.6f +- %.6f]%s' % (step, 'kid' if self.kid_kernel == 'poly3' else 'kid_' + self.kid_kernel,
                                                              out['kid'], out['kid_std'], mark(self.metric == 'kid')))
        if 'authenticity' in out:
            lines.append('[Steps %7d] [authenticity %.4f] [nearest %.4f, real to real %.4f]' % (
                step, out['authenticity'], out['nearest_mean'], out['real_nearest_mean']))
        if 'fd' in out:
            lines.append('[Steps %7d] [fd %.6f] [means %.6f] [tr fake %.6f] [cross %.6f] [tail %.3e]' % (
                step, out['fd'], out['fd_mean_term'], out['fd_trace_fake'], out['fd_cross_term'], out['fd_tail']))
        return lines


def kid_csv_name(kid_kernel):
    """``kid_%d.csv`` for the cubic kernel, ``kid_rq_%d.csv`` for the rational-quadratic one."""
    return 'kid_%d.csv' if kid_kernel == 'poly3' else 'kid_' + kid_kernel + '_%d.csv'


# ---- the training scripts' hook ----
def _refusals(H, P):
    if H.prdc_data and not H.prdc_encoder:
        raise ValueError('--prdc_data needs --prdc_encoder FILE.pt: the metrics are comparable between evaluations only in '
                         'the feature space of ONE frozen encoder, and the discriminator of this run changes at every step')
    if hasattr(P, 'prdc_kid_kernel') and not H.prdc_kid:
        raise ValueError('--prdc_kid_kernel needs --prdc_kid: without it no kernel distance is computed')
    if H.prdc_best == 'kid' and not H.prdc_kid:
        raise ValueError('--prdc_best kid needs --prdc_kid: without it no kernel distance is computed')
    if hasattr(P, 'prdc_fd_iter') and not H.prdc_fd:
        raise ValueError('--prdc_fd_iter needs --prdc_fd: without it no Frechet distance is computed')
    if H.prdc_fd_iter < 1:
        raise ValueError('--prdc_fd_iter must be at least 1, got %r' % (H.prdc_fd_iter,))


HOOK = Hook(
    flags=(('prdc_data', None, dict(type=str, help='npz with x_train uint8 [n, H, W, 3]: rank 0 appends precision / recall / density / coverage of the '
                                                   'generator (g_ema where there is one) against it to prdc_<seed>.csv at every evaluate_every, in '
                                                   'the features of --prdc_encoder; the training trajectory is unchanged')),
           ('prdc_encoder', None, dict(type=str, help='with --prdc_data (required): discriminator checkpoint used as the frozen feature encoder')),
           ('prdc_encoder_arch', None, dict(type=str, help="with --prdc_data: the encoder's architecture (default: the run's)")),
           ('prdc_k', 5, dict(type=int, help='with --prdc_data: neighbours (default: 5)')),
           ('prdc_n', 10000, dict(type=int, help='with --prdc_data: generated images per evaluation (default: 10000; x_train is used whole)')),
           ('prdc_best', None, dict(type=str, choices=BEST_CHOICES,
                                    help='with --prdc_data: keep gen_best.pt / dis_best.pt (and gen_ema_best.pt) of the evaluation with the '
                                         'best value of this metric (the reference keeps these names for its best FID); kid (needs '
                                         '--prdc_kid) is minimised')),
           ('prdc_kid', False, dict(action='store_true',
                                    help='with --prdc_data: every evaluation also appends step,kid,kid_std to kid_<seed>.csv: the kernel '
                                         'distance (cubic kernel, gamma = coef0 = 1, 100 subsets of up to 1000) of the same fake features '
                                         'from the real set, comparable only under one --prdc_encoder file, never with Inception-based KID')),
           ('prdc_kid_kernel', 'poly3', dict(type=str, choices=kid_mod.KERNELS,
                                             help='with --prdc_kid: poly3 (default), or rq: the rational-quadratic mixture (alpha = 1/2, 1, 2; a '
                                                  'characteristic kernel) is computed instead and appended to kid_rq_<seed>.csv, never into '
                                                  'kid_<seed>.csv; --prdc_best kid then tracks that file')),
           ('prdc_auth', False, dict(action='store_true',
                                     help='with --prdc_data: every evaluation also appends step,authenticity,nearest_mean to auth_<seed>.csv: '
                                          'the memorisation check (contrad_amd/nearest.py), the share of the same fakes that is NOT closer to '
                                          'its nearest real image than that image is to its own nearest other real image, and the mean '
                                          'similarity of a fake to its nearest real.  It records only (no --prdc_best choice: not a quantity '
                                          'to maximise); read it against test_nearest.py --holdout, not against 1')),
           ('prdc_fd', False, dict(action='store_true',
                                   help='with --prdc_data: every evaluation also appends step,fd,mean_term,trace_fake,cross_term,tail to '
                                        'fd_<seed>.csv: the Frechet distance (contrad_amd/fd.py) of the same fake features from the real set, '
                                        'comparable only under one --prdc_encoder file, never with Inception-based FID.  It records only: '
                                        '--prdc_best gains no choice for it')),
           ('prdc_fd_iter', fd_mod.N_ITER, dict(type=int, help='with --prdc_fd: Newton-Schulz steps per evaluation, fixed (default: %d)' % fd_mod.N_ITER))),
    switch='prdc_data', refusals=_refusals,
    build=lambda H, run: PRDCMonitor(*run.head, H.prdc_data, H.prdc_encoder, encoder_arch=H.prdc_encoder_arch, k=H.prdc_k, n_fake=H.prdc_n,
                                     best=H.prdc_best, resumed_step=run.resumed_step, P=run.P, kid=H.prdc_kid, kid_kernel=H.prdc_kid_kernel,
                                     auth=H.prdc_auth, fd=H.prdc_fd, fd_iter=H.prdc_fd_iter),
    log_lines=lambda monitor, step, out: monitor.log_lines(step, out),
    improved=lambda out: out['improved'])                              # the reference's best-checkpoint names: this step's networks
add_hook_arguments, check_hook_arguments, hook_options, HOOK_DEFAULTS = HOOK.add_arguments, HOOK.check, HOOK.options, HOOK.defaults


def parse_args(argv=None):
    return features.real_fake_parser(
        'Testing script: precision / recall / density / coverage in the features of a frozen discriminator (one process, '
        'one GPU)',
        'file-name tag and seed of the latents of --gen (default: drawn)',
        before_sizes=(('--k', dict(default=5, type=int, help='neighbours (default: 5)')),)).parse_args(argv)


def main(argv=None):
    P = parse_args(argv)
    return features.real_fake_main(
        P, 'precision / recall / density / coverage run', lambda n_real, n_fake: check_k(P.k, n_real, n_fake),
        lambda E, real, fake, seed: prdc_of(E, real, fake, P.k, P.batch_size),
        lambda out: 'PRDC (k %d): [precision %.4f] [recall %.4f] [density %.4f] [coverage %.4f] on %d fake / %d real images' % (
            out['k'], out['precision'], out['recall'], out['density'], out['coverage'], out['n_fake'], out['n_real']),
        'prdc_%d.json')


if __name__ == '__main__':
    main()
