"""Float64 references of the conv engine's three operations, computed on the GPU without any of the project's kernels:
an im2col GEMM (F.unfold / F.fold + torch.matmul on float64 CUDA tensors, i.e. rocBLAS dgemm), chunked over images so that
the unfolded input stays near 1 GB at any shape.  Tensors in and out are NHWC like the kernels'; the epilogues are those of
include/contrad_hip.h (fwd: gain * lrelu_slope(conv + bias) + addend; dgrad: dx * gain * (act_ref > 0 ? 1 : slope))."""
import torch
import torch.nn.functional as F

_CHUNK_FLOATS = 1 << 27           # 1 GB of float64 per unfolded chunk


def _chunks(N, per_image):
    step = max(1, _CHUNK_FLOATS // max(1, per_image))
    return [(i, min(N, i + step)) for i in range(0, N, step)]


def _w2d(w):
    return w.to(torch.float64).reshape(w.shape[0], -1)          # (K, C * KH * KW), unfold's row order


def fwd(x, w, bias, stride, pad, slope=1.0, gain=1.0, addend=None):
    """x (N,H,W,C), w (K,C,KH,KW) -> y (N,Ho,Wo,K) in float64."""
    N, H, W, C = x.shape
    K, _, KH, KW = w.shape
    Ho, Wo = (H + 2 * pad - KH) // stride + 1, (W + 2 * pad - KW) // stride + 1
    w2 = _w2d(w).to(x.device)
    y = torch.empty(N, Ho, Wo, K, device=x.device, dtype=torch.float64)
    for a, b in _chunks(N, C * KH * KW * Ho * Wo):
        cols = F.unfold(x[a:b].permute(0, 3, 1, 2).to(torch.float64), (KH, KW), padding=pad, stride=stride)
        y[a:b] = torch.matmul(w2, cols).transpose(1, 2).reshape(b - a, Ho, Wo, K)
    if bias is not None:
        y += bias.to(x.device, torch.float64)
    if slope != 1.0:
        y = torch.where(y > 0, y, y * slope)
    y *= gain
    if addend is not None:
        y += addend.to(torch.float64)
    return y


def dgrad(gy, w, x_hw, stride, pad, act_ref=None, slope=1.0, gain=1.0):
    """gy (N,Ho,Wo,K), w (K,C,KH,KW) -> dx (N,H,W,C) in float64 (the transposed convolution, col2im)."""
    N, Ho, Wo, K = gy.shape
    _, C, KH, KW = w.shape
    H, W = x_hw
    w2t = _w2d(w).to(gy.device).t()
    dx = torch.empty(N, H, W, C, device=gy.device, dtype=torch.float64)
    for a, b in _chunks(N, C * KH * KW * Ho * Wo):
        g = gy[a:b].to(torch.float64).reshape(b - a, Ho * Wo, K).transpose(1, 2)
        cols = torch.matmul(w2t, g)
        dx[a:b] = F.fold(cols, (H, W), (KH, KW), padding=pad, stride=stride).permute(0, 2, 3, 1)
    if act_ref is not None:
        one = torch.ones((), device=gy.device, dtype=torch.float64)
        dx *= torch.where(act_ref.to(torch.float64) > 0, one * gain, one * (gain * slope))    # (no act_ref: no act' at all)
    return dx


def wgrad(x, gy, KH, KW, stride, pad):
    """x (N,H,W,C), gy (N,Ho,Wo,K) -> (dw (K,C,KH,KW), dbias (K,)) in float64."""
    N, H, W, C = x.shape
    _, Ho, Wo, K = gy.shape
    dw = torch.zeros(K, C * KH * KW, device=x.device, dtype=torch.float64)
    for a, b in _chunks(N, C * KH * KW * Ho * Wo):
        cols = F.unfold(x[a:b].permute(0, 3, 1, 2).to(torch.float64), (KH, KW), padding=pad, stride=stride)
        g = gy[a:b].to(torch.float64).reshape(b - a, Ho * Wo, K).transpose(1, 2)
        dw += torch.matmul(g, cols.transpose(1, 2)).sum(0)
    return dw.reshape(K, C, KH, KW), gy.to(torch.float64).sum((0, 1, 2))


def errors(out, ref):
    """(max-norm error max|e| / max|ref|, rel-L2 error ||e||_2 / ||ref||_2) of a float32 result against a float64 reference."""
    e = out.to(torch.float64) - ref.to(out.device)
    rmax = ref.abs().max().clamp_min(1e-300)
    rl2 = ref.norm().clamp_min(1e-300)
    return (e.abs().max() / rmax).item(), (e.norm() / rl2).item()
