"""GPU parity of the linear-evaluation head (csrc/linhead.hip) against float64 (tests/linhead_ref64.py: plain float64
torch, none of this project's kernels), every call through contrad_amd.ops:
  * operands are views inside NaN-filled storage, every sentinel must still be NaN afterwards (the Guard pattern of
    tests/test_dstep_kernels_gpu.py); features are strided views, so a read past a row shows up as a NaN;
  * each case names the launch form (K-splits, classes per thread of the logits kernel, 64-row tiles) it is meant to
    reach, and test_launch_forms asserts through the plan query that these are the forms taken;
  * per tensor: max-norm error max|e| / max|ref| below the 1e-3 contract, and both it and the rel-L2 error below a
    per-family bound (FAMILY_TOL: about 5x the worst observed on an MI355X over this module), recorded through
    ``margin``.
Yardstick that does not come from the code under test: the same iteration in fp32 torch on the CPU has worst max-norm
errors 5.1e-7 (logits), 2.1e-7 (loss), 7.3e-7 (gradW), 4.7e-7 (gradb), 5.6e-7 (W after 20 iterations).
"""
import math

import pytest
import torch

import kernel_ledger as L
import linhead_ref64 as R
from contrad_amd import ops
from contrad_amd.evaluate.classifier import test_classifier as run_test_classifier
from contrad_amd.models.gan import get_architecture
from contrad_amd.models.gan.base import LinearWrapper

pytestmark = pytest.mark.gpu

DEV = 'cuda'
NAN = float('nan')
CONTRACT = 1e-3
f64 = torch.float64

# per-family bounds against float64, about 5x the worst observed on an MI355X over this module
FAMILY_TOL = {                  # family: (max-norm, rel-L2)      observed worst (max-norm, rel-L2)
    'logits': (1e-6, 8e-7),                     # 2.0e-7, 1.6e-7
    'loss': (3.5e-7, 3.5e-7),                   # 6.6e-8 (a scalar: one figure)
    'dlogits': (7e-7, 3.7e-7),                  # 1.3e-7, 7.3e-8
    'gradW': (2.8e-6, 1.6e-6),                  # 5.6e-7, 3.2e-7
    'gradb': (3.6e-6, 3.2e-6),                  # 7.2e-7, 6.5e-7   (a draw whose gradb cancels: see SEEDS)
    'W': (1e-6, 3.6e-7),                        # 2.0e-7, 7.2e-8
    'b': (2.4e-6, 1.4e-6),                      # 4.7e-7, 2.8e-7
    'traj_W': (2.8e-6, 6e-7),                   # 5.6e-7, 1.2e-7   (20 iterations)
    'traj_b': (3e-6, 3.2e-6),                   # 6.1e-7, 6.4e-7
    'traj_loss': (3e-7, 2.1e-7),                # 5.1e-8, 4.2e-8
    'module_grad': (5e-6, 2.2e-6),              # 1.0e-6, 4.5e-7
    'classifier': (1e-6, 1e-6),                 # 2.0e-7 (a scalar: one figure)
}


def errors(out, ref):
    ref = ref.to(out.device, f64)
    e = out.to(f64) - ref
    return (e.abs().max() / ref.abs().max().clamp_min(1e-300)).item(), (e.norm() / ref.norm().clamp_min(1e-300)).item()


def check(margin, family, out, ref):
    emax, el2 = errors(out, ref)
    assert emax < CONTRACT, (family, emax)
    margin('linhead %s max-norm' % family, emax, FAMILY_TOL[family][0])
    margin('linhead %s rel-L2' % family, el2, FAMILY_TOL[family][1])


class Guard(object):
    """A dense operand of ``shape`` with ``pad`` NaN elements either side (pad = 4 floats keeps 16-byte alignment)."""

    def __init__(self, shape, pad=4, fill=None, dtype=torch.float32):
        n = math.prod(shape)
        self.buf = torch.full((n + 2 * pad,), NAN, device=DEV, dtype=dtype)
        self.view = self.buf[pad:pad + n].view(*shape)
        self.pad, self.n = pad, n
        if fill is not None:
            self.view.copy_(fill)

    def intact(self):
        return bool(torch.isnan(self.buf[:self.pad]).all() and torch.isnan(self.buf[self.pad + self.n:]).all())


def strided(x2d, ld, c0=0):
    """x2d as rows of stride ld inside a NaN-filled buffer, starting c0 floats in."""
    M, K = x2d.shape
    buf = torch.full(((M + 1) * ld + c0,), NAN, device=DEV)
    v = buf.as_strided((M, K), (ld, 1), c0)
    v.copy_(x2d)
    return v


def gen(seed):
    return torch.Generator().manual_seed(seed)


def draw(N, K, C, seed, scale=2.0):
    g = gen(seed)
    F = torch.randn(N, K, generator=g).relu() * scale / K ** 0.5
    bound = 1.0 / K ** 0.5
    W = (torch.rand(C, K, generator=g) * 2 - 1) * bound              # nn.Linear's default init
    b = (torch.rand(C, generator=g) * 2 - 1) * bound
    y = torch.randint(0, C, (N,), generator=g)
    return F, W, b, y


def learnable(N, K, C, seed):
    """The fixed learnable problem of the trajectory test: one batch, teacher labels."""
    g = gen(seed)
    X = torch.randn(N, K, generator=g).relu() * 4 / K ** 0.5
    y = ((X - X.mean(0)).double() @ torch.randn(C, K, generator=g).double().t()).argmax(1)
    bound = 1.0 / K ** 0.5
    return X, (torch.rand(C, K, generator=g) * 2 - 1) * bound, (torch.rand(C, generator=g) * 2 - 1) * bound, y


def run_iteration(F, W, b, y, lr, ldf=None, c0=0, pad=4):
    """One training iteration through ops inside guarded storage; returns the device tensors and the guards."""
    N, K = F.shape
    C = W.shape[0]
    Fd = strided(F.to(DEV), K if ldf is None else ldf, c0)
    G = {'W': Guard((C, K), pad, W), 'b': Guard((C,), pad, b), 'logits': Guard((N, C), pad), 'dlogits': Guard((N, C), pad),
         'gradW': Guard((C, K), pad), 'gradb': Guard((C,), pad), 'meters': Guard((4,), 1, torch.zeros(4, dtype=f64), dtype=f64),
         'lr': Guard((1,), pad, torch.tensor([lr]))}
    ops.linhead_fwd(Fd, G['W'].view, G['b'].view, y=y.to(DEV), logits=G['logits'].view, dlogits=G['dlogits'].view,
                    meters=G['meters'].view)
    ops.linhead_wgrad_sgd(Fd, G['dlogits'].view, G['W'].view, G['b'].view, lr=G['lr'].view, grad_weight=G['gradW'].view,
                          grad_bias=G['gradb'].view)
    torch.cuda.synchronize()
    return Fd, G


def check_hits(meters, ref, y, N):
    """Hit counts equal the float64 reference's on every row that is not a near-tie; near-ties are capped at 1 %."""
    near = R.near_tie_rows(ref['logits'], y)
    n_near = int(near.sum())
    assert n_near <= max(0.01 * N, 0) or n_near == 0, (n_near, N)
    m = meters.cpu().tolist()
    assert abs(m[1] - ref['hits1'].sum().item()) <= n_near and abs(m[2] - ref['hits5'].sum().item()) <= n_near, (m, n_near)
    assert m[3] == N


# (N, K, C, ldf - K, c0, feature scale): launch form (K-splits, classes per thread, row tiles, classes per thread of the
# weight gradient).  The two kernels are templates over the classes per thread -- linhead_logits_kernel<1..8>,
# linhead_wgrad_kernel<1..4> -- and the cases below reach all twelve (tests/kernel_ledger.py).
CASES = [
    ((256, 8192, 10, 0, 0, 2.0), (128, 1, 4, 1)),      # CIFAR-10 batch: one 64-wide chunk per split, 512 blocks
    ((256, 8192, 100, 0, 0, 2.0), (64, 7, 4, 4)),      # CIFAR-100 batch: two chunks per split (partials stay below F)
    ((80, 8192, 10, 0, 0, 2.0), (128, 1, 2, 1)),       # CIFAR's last train batch at 256: a partial second row tile
    ((16, 8192, 100, 0, 0, 2.0), (64, 7, 1, 4)),       # CIFAR's last test batch at 256
    ((1, 8192, 10, 0, 0, 2.0), (128, 1, 1, 1)),        # a single row
    ((250, 512, 100, 0, 0, 2.0), (4, 7, 4, 4)),        # snresnet18 features: few chunks, ragged last row tile
    ((37, 300, 7, 0, 0, 2.0), (5, 1, 1, 1)),           # K not a multiple of the chunk (ragged last chunk), odd C
    ((5, 8192, 128, 0, 0, 2.0), (64, 8, 1, 4)),        # the widest head
    ((256, 8192, 10, 8, 4, 2.0), (128, 1, 4, 1)),      # ldf > K, 16-byte aligned: vector loads on strided rows
    ((37, 301, 7, 2, 1, 2.0), (5, 1, 1, 1)),           # ldf > K, odd K and misaligned base: the scalar load path
    ((256, 8192, 10, 0, 0, 90.0), (128, 1, 4, 1)),     # unnormalised post-ReLU-like features (|x|^2 of about 4000)
    # the template instances between the narrowest and the widest head: 70 rows (a ragged second row tile), K = 200 (a ragged
    # last chunk), two or four K-splits
    ((70, 200, 20, 0, 0, 2.0), (4, 2, 2, 1)),        # logits<2>
    ((70, 200, 40, 0, 0, 2.0), (4, 3, 2, 2)),        # logits<3>, wgrad<2>
    ((70, 200, 64, 0, 0, 2.0), (2, 4, 2, 2)),        # logits<4>: every class slot of the 16 x 4 layout is a class
    ((70, 200, 72, 0, 0, 2.0), (2, 5, 2, 3)),        # logits<5>, wgrad<3>
    ((70, 200, 72, 3, 1, 2.0), (2, 5, 2, 3)),        # ... on rows of odd stride from a misaligned base: the scalar loads
    ((70, 200, 96, 0, 0, 2.0), (2, 6, 2, 3)),        # logits<6>
    # fewer than five classes (AFHQ has three): every valid row is a top-5 hit; one class: loss 0 and dlogits 0 exactly
    ((70, 200, 1, 0, 0, 2.0), (4, 1, 2, 1)),
    ((70, 200, 2, 0, 0, 2.0), (4, 1, 2, 1)),
    ((70, 200, 3, 0, 0, 2.0), (4, 1, 2, 1)),
]


# Inputs are drawn with seed N + K + C, but for the draws named here.  (70, 200, 2) at its default seed 272 has a bias gradient
# that cancels 221-fold (sum |dlogits| over the rows / |gradb|; the module's other draws stay below 8): against float64 the
# kernel's gradb is then 7.4e-6 off in max-norm and the same sum in fp32 torch on the CPU 4.7e-6 (autograd) / 3.0e-6 (an explicit
# column sum) -- the input's conditioning, not a property of the kernel, so the case draws a batch that cancels 3.4-fold
# and the bound stays.  test_single_iteration asserts the cancellation of every 70-row draw from the float64 reference alone.
SEEDS = {(70, 200, 2): 2}
MAX_CANCELLATION = 8.0


def test_launch_forms():
    for (N, K, C, _dl, _c0, _s), form in CASES:
        assert ops.linhead_plan(N, K, C) == form[:3], (N, K, C)
        assert L.linhead_plan(N, K, C) == form, (N, K, C)            # (ct3 has no library query: the host rule restated)
        S = form[0]
        want = 4 * (64 + 4 * N + S * N * C)           # counter line, per-row scratch, partial sums
        assert ops.lib().raw('contrad_linhead_workspace_bytes')(N, K, C) == want
    assert ops.linhead_plan(256, 8192, 10) == ops.linhead_plan(256, 8192, 10)      # a pure function of (N, K, C)


# (ids: the case and the three plan-query figures of its form, as before the forms carried ct3)
@pytest.mark.parametrize('case,form', CASES, ids=lambda v: 'x'.join(str(i) for i in (v[:3] if len(v) == 4 else v)))
def test_single_iteration(case, form, margin):
    N, K, C, dld, c0, scale = case
    assert ops.linhead_plan(N, K, C) == form[:3]
    F, W, b, y = draw(N, K, C, seed=SEEDS.get((N, K, C), N + K + C), scale=scale)
    ref = R.head_ref64(F, W, b, y, lr=0.1)
    if N == 70 and C > 1:
        assert ref['dlogits'].abs().sum(0).max() < MAX_CANCELLATION * ref['gradb'].abs().max()
    Fd, G = run_iteration(F, W, b, y, 0.1, ldf=K + dld, c0=c0)
    for name in ('logits', 'dlogits', 'gradW', 'gradb', 'W', 'b'):
        check(margin, name, G[name].view, ref[name])
    m = G['meters'].view.cpu()
    if C == 1:                                       # log-sum-exp of one logit is the logit: nothing to round
        assert ref['loss'].item() == 0 and m[0].item() == 0 and bool((G['dlogits'].view == 0).all())
    else:
        margin('linhead loss max-norm', abs(m[0].item() / N - ref['loss'].item()) / abs(ref['loss'].item()), FAMILY_TOL['loss'][0])
    if N < 100:                                      # check_hits allows no near-tie row below 100 rows: the draw has none
        assert int(R.near_tie_rows(ref['logits'], y).sum()) == 0
    check_hits(G['meters'].view, ref, y, N)
    if C < 5:                                        # at most four logits can be above the label's
        assert ref['hits5'].sum().item() == N and m[2].item() == N
    for name, gd in G.items():
        assert gd.intact(), name
    assert float(G['lr'].view) == pytest.approx(0.1, rel=1e-7)


@pytest.mark.parametrize('N,K,C', [(256, 8192, 10), (256, 8192, 100), (250, 512, 100), (37, 8192, 10)])
def test_trajectory(N, K, C, margin):
    """20 iterations on a fixed learnable batch, lr 0.1 for 10 iterations then 0.01 through the device lr."""
    X, W0, b0, y = learnable(N, K, C, seed=N + C)
    W, b, ref_loss, ref_hits = W0.double(), b0.double(), [], []
    for it in range(20):
        r = R.head_ref64(X, W, b, y, lr=0.1 if it < 10 else 0.01)
        ref_loss.append(r['loss'].item()); ref_hits.append(r)
        W, b = r['W'], r['b']
    assert all(ref_loss[i + 1] < ref_loss[i] for i in range(19)), ref_loss        # the reference falls strictly
    Xd, yd = X.to(DEV), y.to(DEV)
    Wd, bd = Guard((C, K), 4, W0), Guard((C,), 4, b0)
    dl, lr, meters = torch.empty(N, C, device=DEV), torch.empty(1, device=DEV), torch.zeros(4, dtype=f64, device=DEV)
    seen, near_total, h1_ref, h5_ref = [], 0, 0.0, 0.0
    for it in range(20):
        lr.fill_(0.1 if it < 10 else 0.01)
        ops.linhead_fwd(Xd, Wd.view, bd.view, y=yd, dlogits=dl, meters=meters, want_logits=False)
        ops.linhead_wgrad_sgd(Xd, dl, Wd.view, bd.view, lr=lr)
        seen.append(meters.clone())
        near_total += int(R.near_tie_rows(ref_hits[it]['logits'], y).sum())
        h1_ref += ref_hits[it]['hits1'].sum().item(); h5_ref += ref_hits[it]['hits5'].sum().item()
    torch.cuda.synchronize()
    sums = torch.stack(seen).cpu()
    losses = torch.cat([sums[:1, 0], sums[1:, 0] - sums[:-1, 0]]) / N
    check(margin, 'traj_loss', losses, torch.tensor(ref_loss, dtype=f64))
    check(margin, 'traj_W', Wd.view, W)
    check(margin, 'traj_b', bd.view, b)
    assert near_total <= 0.01 * 20 * N, near_total
    final = sums[-1].tolist()
    assert abs(final[1] - h1_ref) <= near_total and abs(final[2] - h5_ref) <= near_total and final[3] == 20 * N
    margin('linhead traj_loss max-norm', abs(final[0] / N - sum(ref_loss)) / sum(ref_loss), FAMILY_TOL['traj_loss'][0])
    assert Wd.intact() and bd.intact()


def test_exact_ties_follow_the_strictly_greater_rule():
    """Duplicated weight rows give bitwise-equal logits: a label tied with the maximum is a top-1 hit; a label with
    five equal logits and one larger one is a top-5 hit (only one logit is strictly greater), not a top-1 hit."""
    g = gen(3)
    K = 256
    F = torch.randn(6, K, generator=g).relu()
    w = torch.randn(K, generator=g) * 0.05
    W = torch.stack([w, w, w, w, w, w, w + 0.01 * F[0].sign().abs()])            # class 6 is larger on every row with mass
    b = torch.zeros(7)
    y = torch.tensor([0, 3, 5, 6, 2, 1])
    ref = R.head_ref64(F, W, b, y)
    assert ref['hits1'].tolist() == [0, 0, 0, 1, 0, 0] and ref['hits5'].sum().item() == 6
    meters = torch.zeros(4, dtype=f64, device=DEV)
    lg, _ = ops.linhead_fwd(F.to(DEV), W.to(DEV), b.to(DEV), y=y.to(DEV), meters=meters)
    assert torch.equal(lg[:, 0], lg[:, 5]) and bool((lg[:, 6] > lg[:, 0]).all())
    assert meters.cpu().tolist()[1:] == [1.0, 6.0, 6.0]
    W2 = torch.stack([w, w, w])                                                   # all tied: everything is a top-1 hit
    meters.zero_()
    ops.linhead_fwd(F.to(DEV), W2.to(DEV), None, y=torch.tensor([0, 1, 2, 0, 1, 2], device=DEV), meters=meters)
    assert meters.cpu().tolist()[1:] == [6.0, 6.0, 6.0]


def test_out_of_range_labels_are_handled(margin):
    N, K, C = 40, 512, 10
    F, W, b, y = draw(N, K, C, seed=5)
    y[3], y[17], y[39] = -1, C, 1 << 40
    with pytest.raises(RuntimeError):
        ops.linhead_fwd(F.to(DEV), W.to(DEV), b.to(DEV), y=y)                     # host labels: refused before launch
    ref = R.head_ref64(F, W, b, y, lr=0.1)
    assert ref['loss_rows'][3] == 0 and ref['dlogits'][17].abs().max() == 0
    Fd, G = run_iteration(F, W, b, y, 0.1)                                        # device labels: handled in the kernel
    for name in ('logits', 'dlogits', 'gradW', 'gradb', 'W', 'b'):
        check(margin, name, G[name].view, ref[name])
    assert bool((G['dlogits'].view[[3, 17, 39]] == 0).all())
    m = G['meters'].view.cpu().tolist()
    assert abs(m[0] / N - ref['loss'].item()) < 2e-6 * abs(ref['loss'].item()) and m[3] == N
    assert m[1] == ref['hits1'].sum().item() and m[2] == ref['hits5'].sum().item()
    for name, gd in G.items():
        assert gd.intact(), name


@pytest.mark.parametrize('N,K,C', [(256, 8192, 100), (80, 8192, 10), (37, 300, 7)])
def test_bitwise_repeatable(N, K, C):
    F, W, b, y = draw(N, K, C, seed=11)
    runs = []
    for _ in range(2):
        _Fd, G = run_iteration(F, W, b, y, 0.1)
        runs.append({k: v.view.clone() for k, v in G.items()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_argument_checks():
    F, W, b, y = (t.to(DEV) for t in draw(8, 64, 10, seed=1))
    with pytest.raises(RuntimeError):
        ops.linhead_fwd(F, torch.zeros(129, 64, device=DEV), None)                # C > 128
    with pytest.raises(RuntimeError):
        ops.linhead_fwd(F, W, b, meters=torch.zeros(4, dtype=f64, device=DEV))    # meters without labels
    with pytest.raises(RuntimeError):
        ops.linhead_fwd(F, W, b, y=y.int())
    with pytest.raises(RuntimeError):
        ops.linhead_wgrad_sgd(F, torch.zeros(8, 10, device=DEV))                  # nothing to compute


@pytest.mark.parametrize('N,K,C', [(48, 512, 10), (256, 8192, 100)])
def test_linear_wrapper_forward_backward(N, K, C, margin):
    F, W, b, y = draw(N, K, C, seed=21)
    head = LinearWrapper(K, C)
    with torch.no_grad():
        head.weight.copy_(W); head.bias.copy_(b)
    head = head.to(DEV)
    x = F.to(DEV).requires_grad_()
    out = head(x, None)
    assert out.shape == (N, C)
    loss = torch.nn.functional.cross_entropy(out, y.to(DEV))
    loss.backward()
    x64, W64, b64 = F.double().requires_grad_(), W.double().requires_grad_(), b.double().requires_grad_()
    l64 = torch.nn.functional.cross_entropy(x64 @ W64.t() + b64, y)
    l64.backward()
    check(margin, 'logits', out.detach(), (x64 @ W64.t() + b64).detach())
    check(margin, 'module_grad', head.weight.grad, W64.grad)
    check(margin, 'module_grad', head.bias.grad, b64.grad)
    check(margin, 'module_grad', x.grad, x64.grad)
    assert list(head.state_dict().keys()) == ['weight', 'bias']


@pytest.mark.parametrize('arch', ['sndcgan', 'stylegan2'])
def test_replaced_head_forward(arch):
    torch.manual_seed(3)
    _, D = get_architecture(arch, (32, 32, 3))
    D = D.to(DEV).eval()
    x = torch.rand(12, 3, 32, 32, generator=gen(4)).to(DEV)
    with torch.no_grad():
        stock_before, feats_before = D(x), D.penultimate(x)
    _, D2 = get_architecture(arch, (32, 32, 3))
    D2.load_state_dict(D.state_dict())
    D2 = D2.to(DEV).eval()
    D2.linear = LinearWrapper(D2.d_penul, 10).to(DEV)
    with torch.no_grad():
        out = D2(x)
        feats = D2.penultimate(x)
        out_aux, aux = D2(x, penultimate=True, projection=True)
        stock_after = D(x)
    assert out.shape == (12, 10)
    assert torch.equal(feats, feats_before)                       # the trunk is untouched by the new head
    assert torch.equal(out, D2.linear(feats)) and torch.equal(out_aux, out) and torch.equal(aux['penultimate'], feats)
    assert torch.equal(stock_after, stock_before) and stock_before.shape == (12, 1)     # the stock head: bit for bit
    with torch.no_grad():
        _, aux_stock = D(x, projection=True)
    assert torch.equal(aux['projection'], aux_stock['projection'])
    with pytest.raises(NotImplementedError):
        D2(x, y=torch.zeros(12, dtype=torch.long, device=DEV))
    assert sorted(k for k in D2.state_dict() if k.startswith('linear.')) == ['linear.bias', 'linear.weight']


def test_test_classifier_over_a_short_last_batch(margin):
    torch.manual_seed(5)
    _, D = get_architecture('sndcgan', (32, 32, 3))
    D.linear = LinearWrapper(D.d_penul, 10)
    D = D.to(DEV).eval()
    g = gen(6)
    x, y = torch.rand(70, 3, 32, 32, generator=g), torch.randint(0, 10, (70,), generator=g)
    loader = [(x[0:32], y[0:32]), (x[32:64], y[32:64]), (x[64:70], y[64:70])]
    res = run_test_classifier(D, loader, ['loss', 'error@1', 'error@5'])
    with torch.no_grad():
        feats = D.penultimate(x.to(DEV)).cpu()
    ref = R.head_ref64(feats, D.linear.weight.detach().cpu(), D.linear.bias.detach().cpu(), y)
    margin('linhead classifier max-norm', abs(res['loss'] - ref['loss'].item()) / ref['loss'].item(), FAMILY_TOL['classifier'][0])
    near = int(R.near_tie_rows(ref['logits'], y).sum())
    assert abs((100 - res['error@1']) * 0.7 - ref['hits1'].sum().item()) <= near + 1e-9
    assert abs((100 - res['error@5']) * 0.7 - ref['hits5'].sum().item()) <= near + 1e-9
    assert not D.training
