"""The float64 yardstick of eval-mode BatchNorm + ReLU (tests/dstep_ref64.py: bn_relu_eval, the regimes of
bn_eval_inputs) and the trained-like generator state (tests/cddls_ref64.py: trained_like_networks), on the CPU:
  * the yardstick against F.relu(F.batch_norm(...)) in float64 on NCHW data, with and without the column permutation;
  * every regime reaches the mean^2 / var it is named for;
  * plain fp32 torch on every regime's inputs stays below the 1e-3 contract, so the bound the GPU tests derive from it
    (R.bn_eval_bound) is a tighter one than the contract;
  * the two fp32 compositions restated in numpy: (mean, var) as they are -- what contrad_bn_relu_apply_eval computes --
    and the earlier {mean, var + mean^2} with count = 1, which loses 6e-8 mean^2 / var of the variance.  The earlier form
    breaks the contract in regime D and the derived bound in B - F; the as-is form holds the bound everywhere.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cddls_ref64 as C
import dstep_ref64 as R

CONTRACT = 1e-3
BN_FWD_TOL = (1.3e-6, 7e-7)             # FAMILY_TOL['bn_fwd'] of test_dstep_kernels_gpu.py
EPS = 1e-5
M, K = 256, 128
CASES = [(r, wb) for r in R.BN_EVAL_REGIMES for wb in (True, False) if wb or r not in R.BN_EVAL_NEEDS_BIAS]
IDS = ['%s-%s' % (r, 'cb' if wb else 'nocb') for r, wb in CASES]


def ref_of(inp, perm=1):
    return R.bn_relu_eval(inp['x'], inp['cb'], inp['rm'], inp['rv'], inp['gamma'], inp['beta'], EPS, perm)


@pytest.mark.parametrize('perm', [1, 4])
def test_yardstick_is_float64_batch_norm(perm):
    g = torch.Generator().manual_seed(perm)
    N, Cn, H = 3, 12, 5
    rm, rv = torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.01
    cb, gamma, beta = torch.randn(Cn, generator=g), torch.rand(Cn, generator=g) + 0.5, torch.randn(Cn, generator=g)
    if perm == 1:           # a transposed conv without its bias, NCHW; the kernel sees NHWC rows
        x = torch.randn(N, Cn, H, H, generator=g)
        want = F.relu(F.batch_norm(x.double() + cb.double()[None, :, None, None], rm.double(), rv.double(), gamma.double(),
                                   beta.double(), False, 0.0, EPS)).permute(0, 2, 3, 1).reshape(-1, Cn)
        got = R.bn_relu_eval(x.permute(0, 2, 3, 1).reshape(-1, Cn), cb, rm, rv, gamma, beta, EPS)
    else:                   # norm_init: BatchNorm over Cn features = channel * perm + hw, then view(N, C, h, w) read as NHWC
        x = torch.randn(N, Cn, generator=g)
        y = F.relu(F.batch_norm(x.double(), rm.double(), rv.double(), gamma.double(), beta.double(), False, 0.0, EPS))
        want = y.view(N, Cn // perm, perm).permute(0, 2, 1).reshape(N, Cn)
        got = R.bn_relu_eval(x, None, rm, rv, gamma, beta, EPS, perm)
    assert got.dtype == torch.float64 and float((got - want).abs().max()) < 1e-13


@pytest.mark.parametrize('regime,with_bias', CASES, ids=IDS)
def test_regime_reaches_its_ratio_and_fp32_torch_keeps_the_contract(regime, with_bias):
    inp = R.bn_eval_inputs(regime, M, K, 1, with_bias)
    for k in ('x', 'rm', 'rv', 'gamma', 'beta'):
        assert inp[k].dtype == torch.float32
    want = R.BN_EVAL_REGIMES[regime][2]
    ratio = R.bn_eval_ratio(inp)
    assert want / 3 <= ratio <= want * 3, (regime, ratio, want)
    if regime == 'F':
        assert float(inp['rv'][0]) == 0.0 and float(inp['rv'][1]) == np.float32(1e-12) and float(inp['rv'][2]) == np.float32(1e-4)
        assert torch.equal(inp['x'][:, 0::3], (inp['rm'].double() - (inp['cb'].double() if with_bias else 0))
                           .float()[0::3].expand(M, -1))
    if regime == 'G':
        assert float(inp['rm'].abs().min()) > 90 and float(inp['cb'].abs().min()) > 90
    emax, el2 = R.errors(R.bn_relu_eval_fp32(inp, EPS), ref_of(inp))
    print('regime %s %s: ratio %.3g, fp32 torch max-norm %.2e rel-L2 %.2e' % (regime, with_bias, ratio, emax, el2))
    assert emax < CONTRACT / 10         # (9.3e-5 at the most: tenfold room under the contract)


def _compositions(inp):
    """The BN + ReLU output of the two fp32 compositions, every operation rounded to float32 in numpy."""
    f = np.float32
    x, rm, rv, gamma, beta = (inp[k].numpy() for k in ('x', 'rm', 'rv', 'gamma', 'beta'))
    mean = rm if inp['cb'] is None else (rm - inp['cb'].numpy()).astype(f)
    m2 = (mean * mean).astype(f)
    s2 = (rv + m2).astype(f)                                           # what the callers stacked under the mean
    var_present = np.maximum((s2 * f(1.0) - m2).astype(f), f(0))       # count = 1: stats * inv_n, then the difference

    def apply(var):
        rs = (f(1) / np.sqrt((var + f(EPS)).astype(f))).astype(f)
        v = ((((x - mean).astype(f) * rs).astype(f) * gamma).astype(f) + beta).astype(f)
        return torch.from_numpy(np.maximum(v, f(0)))
    return apply(var_present), apply(rv), int((var_present == 0).sum())


@pytest.mark.parametrize('regime,with_bias', CASES, ids=IDS)
def test_the_two_fp32_compositions(regime, with_bias):
    inp = R.bn_eval_inputs(regime, M, K, 1, with_bias)
    ref = ref_of(inp)
    present, direct, zeros = _compositions(inp)
    e_t, e_p, e_d = R.errors(R.bn_relu_eval_fp32(inp, EPS), ref), R.errors(present, ref), R.errors(direct, ref)
    bound = R.bn_eval_bound(BN_FWD_TOL, e_t, regime)
    print('regime %s %s: {mean, var + mean^2} %.2e / %.2e (var = 0 on %d channels), as they are %.2e / %.2e, fp32 torch '
          '%.2e / %.2e' % ((regime, with_bias) + e_p + (zeros,) + e_d + e_t))
    assert e_d[0] < bound[0] and e_d[1] < bound[1], (regime, e_d, bound)
    if regime in 'BCDEF':
        assert e_p[0] > bound[0] and e_p[1] > bound[1], (regime, e_p, bound)
    else:
        assert e_p[0] < bound[0] and e_p[1] < bound[1], (regime, e_p, bound)
    if regime == 'D':
        assert e_p[0] > CONTRACT
    if regime == 'E':
        assert zeros > K // 4           # the variance is below one ulp of mean^2: gone on many channels


@pytest.mark.parametrize('shift,lo,hi', [(1.0, 1e3, 1.2e4), (3.0, 1e4, 9e4)])
def test_trained_like_state_reaches_a_high_ratio(shift, lo, hi):
    """norm_init of the generator the model-level GPU tests run: mean^2 / var of at least 1e3 (about 3e4 within a factor
    of 3 on the second state), every running variance well above eps (the regime of regime C, not of E)."""
    gsd, _ = C.trained_like_networks(shift)
    ratio = C.bn_state_ratio(gsd, 'norm_init')
    print('linear.bias + %g: norm_init max mean^2 / var = %.3g' % (shift, ratio))
    assert lo <= ratio <= hi
    for prefix in ('norm_init', 'main.1', 'main.4', 'main.7'):
        rv = gsd[prefix + '.running_var']
        assert float(rv.min()) > 10 * EPS, prefix
        assert torch.equal(rv, rv.float().double()) and torch.equal(gsd[prefix + '.running_mean'],
                                                                    gsd[prefix + '.running_mean'].float().double())
    # the statistics are the generator's own: its eval-mode output is normalised (unit variance before gamma, beta)
    z = torch.rand(64, 128, generator=torch.Generator().manual_seed(64), dtype=torch.float64) * 2 - 1
    h = F.linear(z, gsd['linear.weight'], gsd['linear.bias'])
    xh = (h - gsd['norm_init.running_mean']) / torch.sqrt(gsd['norm_init.running_var'])
    assert float(xh.mean(0).abs().max()) < 1e-3 and float((xh.var(0, unbiased=False) - 1).abs().max()) < 1e-3
