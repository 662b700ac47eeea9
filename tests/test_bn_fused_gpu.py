"""Generator BatchNorm with the statistics reduce and the running-statistics update in one launch (contrad_bn_batch_stats)
against the separate colstats / bn_running_update calls: the statistics, the output, the running buffers and the batch
counter bitwise equal, in train mode; eval mode unchanged."""
import pytest
import torch

from contrad_amd import ops

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _separate(x, bias, rm, rv, nbt, gamma, beta, perm_hw, out):
    stats = ops.colstats(x, with_sq=True)
    ops.bn_running_update(stats, float(x.shape[0]), bias, 0.1, rm, rv, nbt)
    ops.bn_relu_apply(x, out, stats, float(x.shape[0]), gamma, beta, 1e-5, perm_hw)
    return stats


def _fused(x, bias, rm, rv, nbt, gamma, beta, perm_hw, out):
    stats = ops.bn_batch_stats(x, bias, 0.1, rm, rv, nbt)
    ops.bn_relu_apply(x, out, stats, float(x.shape[0]), gamma, beta, 1e-5, perm_hw)
    return stats


# (rows, channels, perm_hw, conv bias): G_SNDCGAN's four BatchNorms at N = 512 and N = 64, and odd sizes (scalar partial
# kernel, a last partial block that is not full, fewer channels than a block of the reduce)
@pytest.mark.parametrize('M,K,perm_hw,has_bias', [
    (512, 8192, 16, False), (512 * 64, 256, 1, True), (512 * 256, 128, 1, True), (512 * 1024, 64, 1, True),
    (64, 8192, 16, False), (64 * 64, 256, 1, True), (64 * 256, 128, 1, True), (64 * 1024, 64, 1, True),
    (1000, 37, 1, True), (33, 5, 1, False), (70000, 130, 1, True)])
def test_fused_stats_equal_separate_launches(M, K, perm_hw, has_bias):
    g = torch.Generator().manual_seed(M % 977 + K)
    x = (torch.randn(M, K, generator=g) * 1.5 + 0.3).to(DEV)
    bias = torch.randn(K, generator=g).to(DEV) if has_bias else None
    gamma, beta = (torch.rand(K, generator=g) + 0.5).to(DEV), torch.randn(K, generator=g).to(DEV)
    res = []
    for fn in (_separate, _fused):
        rm, rv = torch.linspace(-1, 1, K).to(DEV), torch.linspace(0.5, 2, K).to(DEV)
        nbt = torch.tensor(3, dtype=torch.long, device=DEV)
        out = torch.empty_like(x)
        for _ in range(2):          # two steps: the running buffers are read and written
            stats = fn(x, bias, rm, rv, nbt, gamma, beta, perm_hw, out)
        res.append((stats, out, rm, rv, nbt))
    for a, b in zip(*res):
        assert torch.equal(a, b)
    assert res[1][4].item() == 5


@pytest.mark.parametrize('N', [64, 512])
def test_generator_train_and_eval(N):
    """G_SNDCGAN.forward under no_grad: train mode on the fused launch equals the layer-by-layer separate calls (images,
    running statistics, counters); eval mode reads the running statistics and leaves them alone."""
    from contrad_amd.models.gan import get_architecture
    torch.manual_seed(0)
    G, _ = get_architecture('sndcgan', (32, 32, 3))
    G = G.to(DEV).train()
    z = torch.rand(N, G.nz, generator=torch.Generator().manual_seed(2)).mul(2).sub(1).to(DEV)
    state0 = {k: v.clone() for k, v in G.state_dict().items()}
    with torch.no_grad():
        y_new = G(z).clone()
    state_new = {k: v.clone() for k, v in G.state_dict().items()}

    G.load_state_dict(state0)
    G.invalidate_cache()
    orig = ops.bn_batch_stats

    def separate(x2d, conv_bias, momentum, rm, rv, nbt=None):
        stats = ops.colstats(x2d, with_sq=True)
        ops.bn_running_update(stats, float(x2d.shape[0]), conv_bias, momentum, rm, rv, nbt)
        return stats
    ops.bn_batch_stats = separate
    try:
        with torch.no_grad():
            y_ref = G(z).clone()
    finally:
        ops.bn_batch_stats = orig
    assert torch.equal(y_new, y_ref)
    for k, v in G.state_dict().items():
        assert torch.equal(v, state_new[k]), k
    assert G.norm_init.num_batches_tracked.item() == 1 and not torch.equal(state0['norm_init.running_mean'], state_new['norm_init.running_mean'])

    G.eval()
    with torch.no_grad():
        y_eval = G(z)
    assert torch.isfinite(y_eval).all() and not torch.equal(y_eval, y_new)
    for k, v in G.state_dict().items():
        assert torch.equal(v, state_new[k]), k
