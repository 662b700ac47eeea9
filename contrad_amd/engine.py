"""The eager training steps of the reference loops as reusable functions, their captured twins, and the data-parallel
gradient exchange that replaces DistributedDataParallel's reducer (train_gan.py:311-313).

Eager steps: ``optimizer_step`` is the one tail every eager step ends in (zero_grad -> backward -> gradient exchange ->
fused Adam; captured.CapturedTrainStep._finish is its captured counterpart), ``_d_step`` the one discriminator step
(train_gan.py:153-163, train_stylegan2.py:199-212, train_stylegan2_contraD.py:148-164,218-226 differ in the loss, in
where the fakes come from and in the lazy R1 term); the script loops' generator steps compute their loss and call the
tail on G.

Data parallelism: one process per GPU; each rank owns N_local real images, draws its own fakes and
augmentation parameters; ONE packed RCCL all-gather of embeddings inside the loss (training/gan/contrad.py), then a
SUM all-reduce of the parameter gradients whose 1/world_size is folded into the fused Adam kernel's grad_scale.
The discriminator's backward hands autograd views of two flat buffers (all weight gradients, all bias gradients),
so the exchange is two large collectives over xGMI instead of DDP's 25 MB buckets.
"""
import os

import torch
import torch.distributed as dist

from .captured import CapturedTrainStep, EagerFirst
from .hostio import THROTTLE, upload_into


# Test hook: run every collective code path on a 1-rank process group (set by bench.py --force-dist / tests).
FORCE_DIST = False


def dist_on():
    """True when this process is one rank of a multi-rank job (or the 1-rank test hook is set)."""
    return dist.is_available() and dist.is_initialized() and (dist.get_world_size() > 1 or FORCE_DIST)


class GradAllReducer(object):
    """Sum-all-reduce ``p.grad`` for all params, coalescing gradients that are views of one storage into a single
    collective over the covering span (the HIP discriminators return their weight gradients as views of one flat
    buffer).  Gradients that stay separate small tensors (the ~40 FusedLeakyReLU / head biases of the StyleGAN2
    discriminator: a latency-bound collective each) are packed into ONE staging buffer, reduced together and copied
    back (``torch._foreach_copy_``: two launches instead of 40 collectives)."""

    SMALL = 1 << 18          # floats: spans below 1 MB are packed

    def __init__(self, params):
        self.params = [p for p in params]

    def spans(self):
        groups = {}
        for p in self.params:
            g = p.grad
            if g is None:
                continue
            if not g.is_contiguous():
                raise RuntimeError('GradAllReducer needs contiguous gradients')
            key = g.untyped_storage().data_ptr()
            lo = g.storage_offset()
            hi = lo + g.numel()
            if key in groups:
                t, a, b = groups[key]
                groups[key] = (t, min(a, lo), max(b, hi))
            else:
                groups[key] = (g, lo, hi)
        out = []
        for g, lo, hi in groups.values():
            out.append(g.as_strided((hi - lo,), (1,), lo))
        return out

    def __call__(self):
        if not dist_on():
            return 1
        spans = self.spans()
        small = [t for t in spans if t.numel() < self.SMALL]
        if len(small) > 1:
            stage = torch.cat([t.reshape(-1) for t in small])
            dist.all_reduce(stage)
            torch._foreach_copy_(small, list(torch.split(stage, [t.numel() for t in small])))
            spans = [t for t in spans if t.numel() >= self.SMALL]
        for flat in spans:
            dist.all_reduce(flat)          # SUM; the mean's 1/W goes into Adam's grad_scale
        return dist.get_world_size()


def setup_grad_exchange(D, overlap=True):
    """The data-parallel gradient exchange of a discriminator: returns the reducer to call after the backward, or None
    when the network exchanges everything inside its backward.  ``D_SNDCGAN``: per-layer collectives inside the fused
    backward (all parameters).  ``ResidualDiscriminatorP``: the packed weight gradients are all-reduced from autograd hooks
    as they are produced (heads and the deep levels first -- their exchange hides behind the long high-resolution part of
    the backward), the bias gradients in one packed collective afterwards."""
    if overlap and hasattr(D, 'enable_grad_overlap'):
        rest = D.enable_grad_overlap(OverlappedGradReducer())
        return GradAllReducer(rest) if rest else None
    return GradAllReducer(D.parameters())


class OverlappedGradReducer(object):
    """Gradient exchange overlapped with the backward pass (what DDP's bucketed reducer does for the reference,
    train_gan.py:311-313), at the granularity the fused discriminator backward produces gradients: each layer's
    PACKED weight-gradient slab is all-reduced (SUM, async on RCCL's stream) as soon as its wgrad kernel is enqueued
    -- the three merged head layers (2/3 of D_SNDCGAN's parameters) first, so their exchange hides behind the whole
    trunk backward.  The spectral-norm weight-gradient transform that follows is linear in the packed gradient and
    uses identical weights on every rank, so reducing before it is equivalent to reducing the final gradients."""

    def __init__(self):
        self.handles = []

    def active(self):
        return dist_on() or (dist.is_available() and dist.is_initialized() and getattr(self, 'force', False))

    def reduce_async(self, t):
        if self.active():
            self.handles.append(dist.all_reduce(t, async_op=True))

    def wait(self):
        for h in self.handles:
            h.wait()
        self.handles = []

    def world(self):
        return dist.get_world_size() if self.active() else 1


def sample_generator(G, num_samples, enable_grad=True):
    """_sample_generator of train_gan.py:96-100."""
    latent = G.sample_latent(num_samples)
    with torch.set_grad_enabled(enable_grad):
        return G(latent)


def set_grad(model, flag=True):
    """utils.set_grad (utils.py:125-127)."""
    for p in model.parameters():
        p.requires_grad = flag


def optimizer_step(opt, loss, net, reducer=None):
    """The tail of every eager step: zero_grad -> backward -> [gradient all-reduce] -> fused Adam with the data-parallel
    mean's 1/W as its grad_scale.  ``net``: the network ``opt`` updates; one that exchanged its gradients inside the
    backward (``_grad_comm``, overlapped) only reports the world size, else ``reducer`` (or None) exchanges them now.
    The eager counterpart of captured.CapturedTrainStep._finish."""
    opt.zero_grad()
    loss.backward()
    comm = getattr(net, '_grad_comm', None)
    world = comm.world() if comm is not None else (reducer() if reducer is not None else 1)
    opt.step(grad_scale=1.0 / world) if world > 1 else opt.step()


def _d_step(P, D, opt_D, options, images, loss_fn, draw_fakes, reducer, r1=False):
    """The eager discriminator step: draw_fakes() -> loss_fn -> [R1 on its own D call] -> zero_grad -> backward ->
    [gradient exchange] -> Adam.  Returns (d_loss, aux); aux['r1'] with ``r1``."""
    THROTTLE.begin()                          # host stays at most one step ahead of the GPU (hostio.py)
    d_loss, aux = loss_fn(P, D, options, images, draw_fakes())
    loss = d_loss + aux['penalty']
    if r1:
        loss = _add_r1(P, D, images, loss, aux)
    optimizer_step(opt_D, loss, D, reducer)
    THROTTLE.end()
    return d_loss, aux


def d_step(P, G, D, opt_D, options, images, reducer=None):
    """One discriminator step, exactly train_gan.py:153-163 (minus the four logging .item() syncs)."""
    return _d_step(P, D, opt_D, options, images, loss_fn=P.train_fn["D"], reducer=reducer,
                   draw_fakes=lambda: sample_generator(G, images.size(0), enable_grad=False))


# ----------------------------------------------------------------------------------------------------------
# StyleGAN2 discriminator steps
# ----------------------------------------------------------------------------------------------------------
def r1_loss(D, images, augment_fn):
    """r1_loss (train_stylegan2.py:106-113): mean_n sum_chw (d D(aug(x)) / d aug(x))^2, differentiable in D's
    parameters (double backward through the HIP op family of contrad_amd.autograd_ops)."""
    from . import autograd_ops as A
    images_aug = augment_fn(images).detach()
    images_aug.requires_grad = True
    d_real = D(images_aug)
    with A.input_grad_only():        # this backward is asked for d / d images only: skip the parameter gradients
        grad_real, = torch.autograd.grad(outputs=d_real.sum(), inputs=images_aug, create_graph=True, retain_graph=True)
    return A.SumSqMeanFn.apply(grad_real)          # grad_real.pow(2).reshape(N, -1).sum(1).mean(), two launches


def _sg2_fakes(G, N, style_mix):
    """G(G.sample_latent(N), style_mix) (train_stylegan2.py:116-123); contrad_amd's Generator draws everything random of
    that forward in one device launch (Generator.draw_inputs), any other generator goes through the reference API."""
    if hasattr(G, 'draw_inputs'):
        return G(**G.draw_inputs(N, style_mix))
    return G(G.sample_latent(N), style_mix=style_mix)


def _add_r1(P, D, images, loss, aux):
    """loss + (0.5 * lbd_r1) * r1 * d_reg_every, the (lazy) R1 term of the StyleGAN2 D-steps, eager and captured, in one
    launch (and one in the backward); the penalty itself goes into aux['r1']."""
    aux['r1'] = r1_loss(D, images, P.augment_fn)
    return torch.add(loss, aux['r1'], alpha=(0.5 * P.lbd_r1) * P.d_reg_every)


def _sg2_d_step(loss_fn, P, G, D, opt_D, options, images, step, reducer, style_mix, fakes, r1):
    """What the two StyleGAN2 D-steps share: the given fakes or fresh ones under no_grad, R1 when asked for and due."""
    def draw_fakes():
        if fakes is not None:
            return fakes
        with torch.no_grad():
            return _sg2_fakes(G, images.size(0), style_mix)

    return _d_step(P, D, opt_D, options, images, loss_fn=loss_fn, draw_fakes=draw_fakes, reducer=reducer,
                   r1=r1 and (step % P.d_reg_every == 0) and P.lbd_r1 > 0)


def d_step_stylegan2(P, G, D, opt_D, options, images, step, reducer=None, style_mix=0.9, *, fakes=None, r1=True):
    """D-step of train_stylegan2.py:199-212 (BASELINE config 4): single 3N-image D call via loss_D_fn, plus the
    R1 penalty every ``P.d_reg_every`` steps weighted (0.5*lbd_r1)*r1*d_reg_every (``--no_lazy`` => every step).
    ``fakes``: the generator step's (detached), as the script feeds them, instead of fresh ones; ``r1=False``: the extra
    critic iterations, which carry no R1 term."""
    return _sg2_d_step(P.train_fn["D"], P, G, D, opt_D, options, images, step, reducer, style_mix, fakes, r1)


# One discriminator call over [two real views | fakes] with the minibatch-stddev groups kept inside each segment (True, the
# product path: D.call_merged) or the reference's two calls; the switch serves the same-box A/B runs of bench.py (tools/dev/r5d.sh, profiles/r05_ab_merged_demod.txt).
_MERGED_CALLS = os.environ.get('CONTRAD_DEV_MERGED', '1') != '0'


def loss_D_fn_separate(P, D, options, images, gen_images):
    """ContraD discriminator loss with the call structure of train_stylegan2_contraD.py (G_D.forward :138-164 and
    _loss_D_fn :95-109): the fakes (N) and the two real views (2N) are augmented SEPARATELY and go through D in two
    calls; the losses act on the concatenated embeddings.  Same return contract as contrad.loss_D_fn."""
    from .training.gan.contrad import _ContraDContrastive, _GanDLoss
    N = images.size(0)
    if _MERGED_CALLS and hasattr(D, 'call_merged') and getattr(P.augment_fn, 'supports_out', False):
        # the two calls as ONE pass over 3N images (only the minibatch-stddev statistics see the call boundary), laid out
        # [real views 2N | fakes N] -- the order the losses want -- by letting each augmentation write its slice of one
        # buffer: no concatenation of the batches, no split + re-concatenation of the outputs (forward and backward).
        # Draw order as in the reference: the fakes' augmentation parameters first, then the real views'.
        both = torch.empty((3 * N,) + tuple(images.shape[1:]), device=images.device, dtype=torch.float32)
        P.augment_fn(gen_images.detach(), out=both[2 * N:])
        P.augment_fn(torch.cat([images, images], dim=0), out=both[:2 * N])
        d_all, aux = D.call_merged(both, [2 * N, N], sg_linear=True, projection=True, projection2=True)
        proj, proj2 = aux['projection'], aux['projection2']
    else:
        aug_f = P.augment_fn(gen_images.detach())                   # (same RNG draw order as the two reference calls)
        aug_r = P.augment_fn(torch.cat([images, images], dim=0))
        if hasattr(D, 'call_batches'):
            (d_gen, aux_g), (d_real2, aux_r) = D.call_batches([aug_f, aug_r], sg_linear=True, projection=True,
                                                              projection2=True)
        else:
            d_gen, aux_g = D(aug_f, sg_linear=True, projection=True, projection2=True)
            d_real2, aux_r = D(aug_r, sg_linear=True, projection=True, projection2=True)
        proj = torch.cat([aux_r['projection'], aux_g['projection']], dim=0)
        proj2 = torch.cat([aux_r['projection2'], aux_g['projection2']], dim=0)
        d_all = torch.cat([d_real2, d_gen], dim=0)
    simclr, sup = _ContraDContrastive.apply(proj, proj2, N, P.temp, bool(P.distributed))
    gan, d_real_m, d_gen_m = _GanDLoss.apply(d_all, N, options['loss'])
    return simclr + P.lbd_a * sup, {'penalty': gan, 'd_real': d_real_m, 'd_gen': d_gen_m}


def d_step_stylegan2_contrad(P, G, D, opt_D, options, images, step, reducer=None, style_mix=0.9, *, fakes=None, r1=True):
    """D-step of train_stylegan2_contraD.py:148-164,218-226 (BASELINE config 5): loss_D_fn_separate + lazy R1 on
    its own D call.  Options as d_step_stylegan2."""
    return _sg2_d_step(loss_D_fn_separate, P, G, D, opt_D, options, images, step, reducer, style_mix, fakes, r1)


# ----------------------------------------------------------------------------------------------------------
# static inputs of the captured steps
# ----------------------------------------------------------------------------------------------------------
class _StaticAugment(object):
    """Stand-in for ``P.augment_fn`` inside a captured step: the k-th call of a step applies the k-th parameter block.
    ``refresh()`` draws every block on the host with the pipeline's own sampler, in call order (the reference's RNG
    order), and hands it into static device memory; the colour-op order travels in column 15 (SimCLRAugment.sample
    writes it), the Gaussian taps of simclr_hq in a static kernel tensor."""

    def __init__(self, aug, sizes, H, W, device):
        from . import ops
        self.aug, self.sizes, self.H, self.W, self.dev = aug, list(sizes), H, W, device
        self.blocks = [torch.zeros(n, ops.AUG_NPARAM, device=device) for n in self.sizes]
        self.radius = int((H // 10) / 2) if aug.p_blur is not None else 0
        self.taps = [torch.zeros(2 * self.radius + 1, device=device) for _ in self.sizes] if self.radius > 0 else None
        self.k = 0

    def refresh(self):
        for i, n in enumerate(self.sizes):
            Pm, _cf, sigma = self.aug.sample(n, self.H, self.W)
            upload_into(Pm, self.blocks[i])
            if self.taps is not None:
                _r, g = self.aug.blur_kernel(self.H, sigma)
                upload_into(g.view(1, -1), self.taps[i].view(1, -1))

    supports_out = True          # (``out=``: the last stage writes into the caller's buffer, see SimCLRAugment.apply)

    def __call__(self, x, out=None):
        from . import ops
        i, self.k = self.k, self.k + 1
        if x.shape[0] != self.sizes[i]:
            raise RuntimeError('captured step: augmentation call %d saw %d images, planned %d' % (i, x.shape[0], self.sizes[i]))
        if x.requires_grad and torch.is_grad_enabled():      # generator step: gradient flows through the augmentation
            from .augment import _SimCLRFn
            if out is not None:
                raise RuntimeError('augmentation: out= is a forward-only option')
            return _SimCLRFn.apply(x.contiguous().float(), self.blocks[i], -1, self.aug.r_c is not None,
                                   (self.radius, self.taps[i]) if self.taps is not None else None,
                                   self.aug.cutout_length if self.aug.p_cutout is not None else None)
        res = ops.simclr_augment(x.detach().contiguous().float(), self.blocks[i], -1, self.aug.r_c is not None,
                                 out=None if self.taps is not None else out)
        if self.taps is not None:
            res = ops.gaussian_blur_masked(res, self.blocks[i], self.taps[i], self.radius, out=out)
        if self.aug.p_cutout is not None:
            ops.cutout_masked_(res, self.blocks[i], self.aug.cutout_length)
        return res


class _StaticSG2Inputs(object):
    """Everything random the StyleGAN2 generator consumes in one forward, as static device tensors: latents, mixing
    latents, mixing layers, per-layer noise.  ``refresh()`` draws them in the forward's own order (device draws for the
    latents and the noise, CPU-generator draws for the mixing mask, generator.py:233-234,252-259,91-92)."""

    def __init__(self, G, N, device, style_mix):
        self.G, self.N, self.dev, self.style_mix = G, N, device, style_mix
        self.flat = torch.zeros(sum(G.input_sizes(N)), device=device)        # z | mixing latent | per-layer noise
        self.mix_layer = torch.zeros(N, device=device)
        self.mixing = G.training and style_mix > 0
        z, z_mix, noise = G.input_views(self.flat, N)
        self.kw = dict(input=z, style_mix=style_mix, noise=noise)
        if self.mixing:
            self.kw['_mix'] = (z_mix, self.mix_layer)

    def refresh(self):
        """Generator.draw_inputs' draws, in its order, into the static tensors: one device normal_(), then the CPU draws."""
        G, N = self.G, self.N
        self.flat.normal_()
        if self.mixing:
            nomix = torch.rand(N) >= self.style_mix
            mix_layer = torch.randint(G.n_latent, (N,)).masked_fill(nomix, G.n_latent)
            upload_into(mix_layer.float().view(-1, 1), self.mix_layer.view(-1, 1))

    def forward(self):
        return self.G(**self.kw)


def _with_augment(P, augment_fn):
    """A copy of the run's namespace whose ``augment_fn`` is the captured step's static stand-in."""
    import argparse
    Pg = argparse.Namespace(**vars(P))
    Pg.augment_fn = augment_fn
    return Pg


# ----------------------------------------------------------------------------------------------------------
# the discriminator steps as captured hipGraphs (protocol and replay: captured.py)
# ----------------------------------------------------------------------------------------------------------
class GraphedDStep(CapturedTrainStep):
    """``d_step`` (train_gan.py:153-163) captured ONCE into a hipGraph and replayed every iteration.

    One D-step is ~120 kernel launches; enqueued from Python they cost ~2.8 ms of host time -- hidden behind 17.7 ms of
    GPU work at batch 512, but most of the 3.5 ms step one rank of an 8-GPU job runs at batch 64.
    Replaying a captured graph takes the host out: per step it only draws the random numbers (latents, augmentation
    parameters -- on the host, in the reference's RNG order, exactly as the eager path), hands them over into STATIC
    device tensors, refreshes three Adam scalars, and launches the graph.  What had to move from launch arguments into
    device memory for that: the colour-op order of the augmentation (column 15 of the parameter block) and Adam's
    step-dependent scalars (``contrad_adam_step_dev``).

    With a process group (one rank of a data-parallel job, train_gan.py:230-318) the collectives are captured WITH the
    step: G's SyncBN statistics all-reduce, the packed embedding all-gather inside the loss and the per-layer gradient
    all-reduces the fused backward overlaps with itself (OverlappedGradReducer: RCCL's own stream forks from and joins the
    capture stream through events, which a stream capture records as graph edges); Adam's 1/W travels in the device
    scalars.  A per-rank batch of 64 is ~3.4 ms of GPU work against ~2.8 ms of Python launch time in the eager path
     -- this is what takes the host off that critical path.  Every rank must replay the same graph
    the same number of times (as every rank must issue the same eager collectives).
    """

    def __init__(self, P, G, D, opt_D, options, images, warmup=3):
        from .augment import SimCLRAugment
        self.P, self.G, self.D, self.options = P, G, D, options
        self.aug = P.augment_fn
        if not isinstance(self.aug, SimCLRAugment) or self.aug.p_blur is not None:
            raise NotImplementedError('GraphedDStep: the simclr pipeline')
        on = dist_on()
        flat = on and getattr(D, '_grad_comm', None) is None        # else: exchanged inside the backward (overlapped)
        super().__init__(opt_D, GradAllReducer(D.parameters()) if flat else None, on, images.device)
        self.images = images.clone()                    # static input: load_images() hands over a new real batch
        self.N = N = images.size(0)
        for _ in range(warmup if len(opt_D.state) else max(warmup, 1)):     # optimizer state, workspaces, pools
            d_step(P, G, D, opt_D, options, images, self.reducer)
        self.z = torch.zeros(N, G.nz, device=images.device)
        self.saug = _StaticAugment(self.aug, [3 * N], images.shape[2], images.shape[3], images.device)
        self._capture(quiesce=(D,), repack=(G,))        # G moves between D-steps in training: the step re-packs its weights

    def load_images(self, images):
        self.images.copy_(images)

    def _refresh_inputs(self):
        z = torch.empty(self.N, self.G.nz).uniform_(-1, 1)              # G.sample_latent's draw (sndcgan.py:50-52)
        upload_into(z, self.z)
        self.saug.refresh()                                             # (drawn after z, as the eager step)

    def _body(self):
        from . import ops
        from .training.gan.contrad import _ContraDContrastive, _GanDLoss
        P, G, D, N = self.P, self.G, self.D, self.N
        with torch.no_grad():
            gen = G(self.z)
            cat = torch.cat([self.images, self.images, gen], dim=0)
            aug = ops.simclr_augment(cat, self.saug.blocks[0], -1, self.aug.r_c is not None)
        d_all, aux = D(aug, sg_linear=True, projection=True, projection2=True)
        simclr, sup = _ContraDContrastive.apply(aux['projection'], aux['projection2'], N, P.temp,
                                                bool(P.distributed) and self.dist)
        gan, d_real, d_gen = _GanDLoss.apply(d_all, N, self.options['loss'])
        d_loss = simclr + P.lbd_a * sup
        return self._finish(d_loss + gan, (d_loss, {'penalty': gan, 'd_real': d_real, 'd_gen': d_gen}))


class GraphedSG2DStep(CapturedTrainStep):
    """The StyleGAN2 D-steps (``d_step_stylegan2`` / ``d_step_stylegan2_contrad``) as ONE captured hipGraph.

    These steps are 500-800 launches of mostly small kernels (the R1 double backward alone builds ~300 nodes); enqueued
    from Python they cost 19-27 ms of host time per step depending on the host core -- the same order as the 19 ms of GPU
    work of BASELINE config 4, which therefore flipped between GPU-bound (20.5 ms) and host-bound (27 ms) from run to run.
    Everything random is drawn OUTSIDE the graph, in the eager path's order -- device draws (latents, mixing latents,
    per-layer noise) into static tensors, host draws (mixing layers, augmentation blocks, blur taps) handed over -- so a
    replay consumes exactly the random numbers the eager step would: ``tests/test_graph_gpu.py`` checks bitwise equality.
    With lazy R1 (``d_reg_every`` > 1) the graph holds the plain step and the R1 steps run eagerly."""

    def __init__(self, P, G, D, opt_D, options, images, contrad_script, style_mix=0.9, warmup=2):
        on = dist_on()              # one rank of a data-parallel job: the embedding all-gather (inside the loss) and the
        reducer = None              # gradient all-reduces (from the backward's hooks and / or after it) are captured
        if on:
            rest = D.overlap_rest() if getattr(D, '_pack_comm', None) is not None else None
            reducer = GradAllReducer(rest if rest is not None else D.parameters())
        super().__init__(opt_D, reducer, on, images.device)
        self.P, self.G, self.D, self.options, self.images = P, G, D, options, images.clone()
        self.contrad_script, self.style_mix = contrad_script, style_mix
        self.eager = d_step_stylegan2_contrad if contrad_script else d_step_stylegan2
        self.N = N = images.size(0)
        self.r1_in_graph = P.lbd_r1 > 0 and P.d_reg_every == 1
        for s in range(1, (warmup if len(opt_D.state) else max(warmup, 1)) + 1):     # optimizer state, workspaces
            self.eager(P, G, D, opt_D, options, images, s if P.d_reg_every == 1 else 1, self.reducer, style_mix)
        sizes = ([N, 2 * N] if contrad_script else [3 * N]) + ([N] if self.r1_in_graph else [])
        self.saug = _StaticAugment(P.augment_fn, sizes, images.shape[2], images.shape[3], images.device)
        self.Pg = _with_augment(P, self.saug)
        self.gin = _StaticSG2Inputs(G, N, images.device, style_mix)
        self._capture(quiesce=(D,), repack=(G,))        # as GraphedDStep: the packed tables are rebuilt inside the step

    def load_images(self, images):
        self.images.copy_(images)

    def _refresh_inputs(self):
        self.gin.refresh()
        self.saug.refresh()

    def _body(self):
        P, D = self.Pg, self.D
        self.saug.k = 0
        with torch.no_grad():
            gen = self.gin.forward()
        if self.contrad_script:
            d_loss, aux = loss_D_fn_separate(P, D, self.options, self.images, gen)
        else:
            d_loss, aux = P.train_fn["D"](P, D, self.options, self.images, gen)
        loss = d_loss + aux['penalty']
        if self.r1_in_graph:
            loss = _add_r1(P, D, self.images, loss, aux)        # (P is self.Pg: the static stand-in augments)
        return self._finish(loss, (d_loss, aux))

    def __call__(self, step):
        P = self.P
        if P.lbd_r1 > 0 and P.d_reg_every > 1 and step % P.d_reg_every == 0:      # lazy-R1 step: eager
            return self.eager(P, self.G, self.D, self.opt, self.options, self.images, step, self.reducer, self.style_mix)
        return super().__call__()


# ----------------------------------------------------------------------------------------------------------
# the generator steps as captured hipGraphs (the other half of a training iteration)
# ----------------------------------------------------------------------------------------------------------
class _GraphedGeneratorStep(CapturedTrainStep):
    """What the two generator steps share.  The caller has set ``set_grad(G, True); set_grad(D, False)`` and both
    networks to train mode, and ``opt_G`` holds state (one eager step has run).  With a process group SyncBN's statistics
    exchange and G's gradient all-reduce are captured with the step."""

    def __init__(self, P, G, D, opt_G, options, N, H, W):
        on = dist_on()
        if not len(opt_G.state):
            raise RuntimeError('%s: capture after the first eager generator step (Adam state)' % type(self).__name__)
        dev = next(G.parameters()).device
        super().__init__(opt_G, GradAllReducer(G.parameters()) if on else None, on, dev)
        self.P, self.G, self.D, self.options, self.N = P, G, D, options, N
        self.saug = _StaticAugment(P.augment_fn, [N], H, W, dev)


class GraphedGStep(_GraphedGeneratorStep):
    """The SNDCGAN generator step (train_gan.py:170-179: fakes WITH gradient -> ``loss_G_fn`` = D(augment(G(z))) ->
    backward through D, the augmentation and G -> Adam on G) as one captured hipGraph.  Per replay the host draws the
    latents and the augmentation block in the eager order."""

    def __init__(self, P, G, D, opt_G, options, N, H, W):
        from .augment import SimCLRAugment
        if not isinstance(P.augment_fn, SimCLRAugment):
            raise NotImplementedError('GraphedGStep: simclr-family pipeline')
        super().__init__(P, G, D, opt_G, options, N, H, W)
        self.Pg = _with_augment(P, self.saug)
        self.z = torch.zeros(N, G.nz, device=self.hyper.device)
        self._capture(quiesce=(D,), repack=(G,))

    def _refresh_inputs(self):
        z = torch.empty(self.N, self.G.nz).uniform_(-1, 1)             # G.sample_latent's draw (sndcgan.py:50-52)
        upload_into(z, self.z)
        self.saug.refresh()

    def _body(self):
        self.saug.k = 0
        gen = self.G(self.z)
        g_loss = self.Pg.train_fn["G"](self.Pg, self.D, self.options, None, gen)
        return self._finish(g_loss, g_loss)


class GraphedSG2GStep(_GraphedGeneratorStep):
    """The StyleGAN2 generator step of train_stylegan2_contraD.py:138-146,207 (D with ``sg_linear=False`` and both
    projections on the augmented fakes, non-saturating loss) as one captured hipGraph; same contract as GraphedGStep."""

    def __init__(self, P, G, D, opt_G, options, N, H, W, style_mix=0.9):
        super().__init__(P, G, D, opt_G, options, N, H, W)
        self.gin = _StaticSG2Inputs(G, N, self.hyper.device, style_mix)
        # (the forward with gradient builds its tables inside the autograd graph and never reads G's cache: invalidating
        # it around this capture changes nothing, so the four steps capture alike)
        self._capture(quiesce=(D,), repack=(G,))

    def _refresh_inputs(self):
        self.gin.refresh()
        self.saug.refresh()

    def _body(self):
        from .training.gan.contrad import _GanGLoss
        self.saug.k = 0
        gen = self.gin.forward()
        d_gen, _aux = self.D(self.saug(gen), sg_linear=False, projection=True, projection2=True)
        g_loss = _GanGLoss.apply(d_gen, 'nonsat')
        return self._finish(g_loss, g_loss)


class GraphedCritic(object):
    """``--graph`` of the train scripts: the D-step and the generator step of an iteration, each replayed from its own
    captured graph.  Each is captured lazily, at its first occurrence the eager-first rule admits (captured.EagerFirst:
    from the second iteration of the process on); until then ``__call__`` / ``generator`` return None and the caller
    runs the step eagerly.  Every replay consumes exactly the host random numbers the eager iteration would, so a run with
    ``--graph`` writes bitwise the checkpoints of a run without (tests/test_graph_gpu.py).  ``make_d(P, G, D, opt_D,
    options, images)`` / ``make_g(P, G, D, opt_G, options, N, H, W)`` build the steps; ``not_contrad``: the error text for
    any other ``P.mode`` (one %s)."""

    def __init__(self, make_d, make_g, not_contrad):
        self.make_d, self.make_g, self.not_contrad = make_d, make_g, not_contrad
        self.step = self.gstep = None
        self.first_d, self.first_g = EagerFirst(), EagerFirst()

    def generator(self, P, opt, G, D, opt_G, images):
        if self.gstep is None:
            if not self.first_g.may_capture(opt_G):
                return None
            self.gstep = self.make_g(P, G, D, opt_G, opt, images.size(0), images.size(2), images.size(3))
        return self.gstep()

    def __call__(self, P, opt, G, D, opt_D, images, *step):
        if self.step is None:
            if not self.first_d.may_capture(opt_D):
                return None
            if P.mode != 'contrad':
                raise NotImplementedError(self.not_contrad % P.mode)
            self.step = self.make_d(P, G, D, opt_D, opt, images)
        self.step.load_images(images)
        return self.step(*step)
