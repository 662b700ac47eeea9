"""Thin, allocation-explicit Python wrappers over the C ABI (include/contrad_hip.h).

Every function takes CUDA fp32 torch tensors purely as device-memory handles (``data_ptr()``) and
launches on ``torch.cuda.current_stream()``, so the calls are safe from both the Python main thread
(forward) and the autograd engine thread (backward) -- the threading contract of SURVEY.md 8(b).
Activations are NHWC: a tensor of shape (N, H, W, C) whose last dim is contiguous; the pixel stride
``stride(2)`` is the leading dimension (allows channel-sliced views of wider buffers).
"""
import ctypes
import math
import os

import torch

from ._lib import ConvDesc, ContrastProblem, FilterBatch, FilterJob, FILTER_MAX_JOBS, L2normProblem, lib


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)


def _stream_handle():
    """Raw hipStream_t of torch's current stream on the current device (the direct C accessor when this torch build has
    it: torch.cuda.current_stream() builds a Stream object per call, ~9 us x 50 launches per step)."""
    if _raw_stream is not None:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _stream():
    return ctypes.c_void_p(_stream_handle())


def _chk(t, name):
    if t is None:
        return
    if not t.is_cuda or t.dtype != torch.float32:
        raise RuntimeError('contrad_hip: %s must be a CUDA float32 tensor (got %s, %s)' % (name, t.device, t.dtype))
    if t.dim() > 0 and t.numel() > 0 and t.stride(-1) != 1:
        raise RuntimeError('contrad_hip: %s must be contiguous in its last dimension' % name)


def _ld(t):
    """Pixel stride of an NHWC (N,H,W,C) view / row stride of a (M,C) matrix."""
    if t.dim() == 4:
        N, H, W, C = t.shape
        ld = t.stride(2) if W > 1 else (t.stride(1) if H > 1 else (t.stride(0) if N > 1 else C))
        if (W > 1 and t.stride(1) != W * ld) or (H * W > 1 and N > 1 and t.stride(0) != H * W * ld):
            raise RuntimeError('contrad_hip: NHWC view must be dense over (N,H,W)')
        return ld
    if t.dim() == 2:
        return t.stride(0) if t.size(0) > 1 else max(t.size(1), t.stride(0))
    raise RuntimeError('contrad_hip: expected a 2-D or 4-D tensor')


def round_up(x, m):
    return (x + m - 1) // m * m


def out_size(h, k, stride, pad):
    return (h + 2 * pad - k) // stride + 1


# Optional per-launch profiler (bench.py): when set to a list, conv-engine launches are bracketed by events on the
# launch stream and appended as (kernel_name, algorithmic_flops, start_event, end_event, layer shape, workgroups of the main launch).  kernel_name is the device
# kernel's name as rocprofv3 prints it.  PROFILE_ONLY (a kernel name) restricts the bracketing to that kernel: every
# event pair costs ~10 us of stream time, so the timed region of bench.py instruments the dominant kernel only.
# (A WGRAD bracket spans the split-K main kernel and its wgrad_reduce_kernel: one C-ABI call launches both.)
PROFILE = None
PROFILE_ONLY = None
# Optional launch log without events (legal inside a stream capture): when set to a list, every conv-engine call appends
# (kernel_name, shape, workgroups, algorithmic GFLOP, executed share); engine.Graphed*Step appends the marker 'capture'
# right before it captures, so bench.py --shape-table can record the launch ORDER of the captured step (a replay keeps the
# order of its capture, which need not be the order of the eager step the event-bracketed table comes from).
SEQUENCE = None


def conv_kernel_name(mode, d):
    bm, bn = ctypes.c_int(0), ctypes.c_int(0)
    lib().call('contrad_conv2d_tile', ctypes.byref(d), mode, ctypes.byref(bm), ctypes.byref(bn))
    path = lib().raw('contrad_conv2d_path')(ctypes.byref(d), mode)
    if path == 4:
        return 'wgrad_c32_kernel'
    if path == 5:
        return 'fwd_k1_kernel'
    if path == 6:
        return 'conv_c32_kernel<%d>' % mode
    if path == 7:
        return 'wino_wgrad_kernel' if mode == 2 else 'wino_kernel<%d>' % mode
    if path == 8:
        return 'wino22_wgrad_kernel' if mode == 2 else 'wino22_kernel<%d>' % mode
    if path == 9:
        return 'wino44_kernel<%d>' % mode
    if path == 11:
        return 'wino44n_kernel<%d>' % mode
    if path == 10:
        return 'wino23_kernel'
    if path in (2, 3):
        return 'igemm_lean_kernel<%d, %d, %d>' % (mode, bm.value, bn.value)
    return 'igemm_kernel<%d, %d, %d, %s>' % (mode, bm.value, bn.value, 'true' if path == 1 else 'false')


def _conv_call(mode, d, name, *args):
    if SEQUENCE is not None:
        SEQUENCE.append([conv_kernel_name(mode, d), [d.N, d.H, d.W, d.C, d.K, d.KH, d.KW, d.stride, d.pad],
                         int(lib().raw('contrad_conv2d_grid_blocks')(ctypes.byref(d), mode, 1)),
                         round(2.0 * d.N * d.Ho * d.Wo * d.K * d.C * d.KH * d.KW / 1e9, 4),
                         round(float(lib().raw('contrad_conv2d_executed_fraction')(ctypes.byref(d), mode)), 4)])
    if PROFILE is None:
        lib().call(name, *args)
        return
    kname = conv_kernel_name(mode, d)
    if PROFILE_ONLY is not None and kname != PROFILE_ONLY:
        lib().call(name, *args)
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream()
    e0.record(st)
    lib().call(name, *args)
    e1.record(st)
    # algorithmic flops; for a strided dgrad this equals the forward count (only contributing taps are multiplied)
    flops = 2.0 * d.N * d.Ho * d.Wo * d.K * d.C * d.KH * d.KW
    shape = (d.N, d.H, d.W, d.C, d.K, d.KH, d.KW, d.stride, d.pad)
    blocks = lib().raw('contrad_conv2d_grid_blocks')(ctypes.byref(d), mode, 1)
    # share of those flops the kernel issues (pixel-major tiles skip the tap-positions that read padding)
    executed = float(lib().raw('contrad_conv2d_executed_fraction')(ctypes.byref(d), mode))
    PROFILE.append((kname, flops, e0, e1, shape, int(blocks), executed))


def make_desc(N, H, W, C, K, KH, KW, stride, pad, ldx, ldy, ldw):
    return ConvDesc(N, H, W, C, ldx, out_size(H, KH, stride, pad), out_size(W, KW, stride, pad), K, ldy,
                    KH, KW, stride, pad, ldw)


def pack_weight(w):
    """(K, C, KH, KW) -> packed GEMM layout [(kh*KW+kw)*C + c][ldw], ldw = round_up(K, 4).  (Host helper for
    tests / one-off packing; the training path packs on device inside the spectral-norm weight prep.)"""
    K, C, KH, KW = w.shape
    ldw = round_up(K, 4)
    wp = w.new_zeros(KH * KW * C, ldw)
    wp[:, :K] = w.permute(2, 3, 1, 0).reshape(KH * KW * C, K)
    return wp


def unpack_weight(wp, K, C, KH, KW):
    return wp[:, :K].reshape(KH, KW, C, K).permute(3, 2, 0, 1).contiguous()


# --------------------------------------------------------------------------------------------------
# convolution engine
# --------------------------------------------------------------------------------------------------
# Transformed Winograd filters made once per weight prep (contrad_conv2d_filter_prep) instead of by every conv call.
# (dev switch, read once: CONTRAD_DEV_FILTER_PREP=0 keeps the networks on the per-call transform, for A/B runs)
FILTER_PREP = os.environ.get('CONTRAD_DEV_FILTER_PREP', '1') != '0'
# (the same for the two other launch mergers of the D-step: both contrastive problems per launch, training/gan/contrad.py;
# the BatchNorm statistics reduce and running update in one launch, models/gan/sndcgan.py)
CONTRAST_PAIR = os.environ.get('CONTRAD_DEV_CONTRAST_PAIR', '1') != '0'
BN_FUSED = os.environ.get('CONTRAD_DEV_BN_FUSED', '1') != '0'


def filter_kind(d, mode):
    """(kind, bytes) of the transformed filter conv2d_fwd (mode 0) / conv2d_dgrad (mode 1) read for descriptor ``d``; kind 0:
    the plan takes a direct kernel."""
    nb = ctypes.c_longlong(0)
    kind = lib().raw('contrad_conv2d_filter_kind')(ctypes.byref(d), mode, ctypes.byref(nb))
    if kind < 0:
        raise RuntimeError('contrad_hip: bad conv descriptor (%d)' % kind)
    return kind, nb.value


def fwd_desc(x_shape, wp, K, KH, KW, stride, pad):
    """Descriptor of conv2d_fwd on a dense NHWC input of ``x_shape`` writing a dense output."""
    N, H, W, C = x_shape
    return make_desc(N, H, W, C, K, KH, KW, stride, pad, C, K, wp.stride(0))


def dgrad_desc(x_shape, wp, K, KH, KW, stride, pad):
    """Descriptor of conv2d_dgrad producing a dense dx of ``x_shape`` from a dense gy with K channels."""
    return fwd_desc(x_shape, wp, K, KH, KW, stride, pad)


class PreparedFilters(object):
    """Transformed Winograd filters of a set of layers, made by ONE launch (``filter_prep``) right after the weight prep
    that packed their weights.  ``get`` hands the job of (mode, packed weight) to the conv call; the C side checks that
    it fits the path the call plans and transforms per call otherwise, so a shape the request list did not foresee
    (another batch size, a strided view) is slower, never wrong.  Holds the U storage: keep it alive until the last
    consumer has been launched (the autograd ctx of D, the pack cache of G)."""

    def __init__(self):
        self.jobs = {}
        self.buf = None

    def get(self, mode, wp):
        return self.jobs.get((mode, wp.data_ptr()))


def filter_prep(requests, device):
    """requests: iterable of (mode, ConvDesc, packed weight).  Allocates the U buffers (one allocation) and fills all of
    them in one launch per FILTER_MAX_JOBS jobs; requests whose plan is not Winograd are dropped.  Allocates: call it where
    the packed weights are allocated, never between launches of a step that must not allocate."""
    pf = PreparedFilters()
    todo, tot = [], 0
    for mode, d, wp in requests:
        kind, nb = filter_kind(d, mode)
        if kind == 0 or (mode, wp.data_ptr()) in pf.jobs:
            continue
        _chk(wp, 'wp')
        j = FilterJob(wp.data_ptr(), 0, kind, mode, d.C, d.K, d.ldw)
        pf.jobs[(mode, wp.data_ptr())] = j
        todo.append((j, tot))
        tot += round_up(nb // 4, 4)
    if not todo:
        return pf
    pf.buf = torch.empty(tot, device=device, dtype=torch.float32)
    base = pf.buf.data_ptr()
    for j, off in todo:
        j.U = base + 4 * off
    for start in range(0, len(todo), FILTER_MAX_JOBS):
        b = FilterBatch()
        chunk = todo[start:start + FILTER_MAX_JOBS]
        b.n = len(chunk)
        for i, (j, _) in enumerate(chunk):
            b.jobs[i] = j
        lib().call('contrad_conv2d_filter_prep', ctypes.byref(b), _stream())
    return pf


def conv2d_fwd(x, wp, bias, K, KH, KW, stride, pad, slope=1.0, gain=1.0, out=None, addend=None, filters=None):
    """x: (N,H,W,C) NHWC; wp packed (KH*KW*C, ldw); returns y (N,Ho,Wo,K) = gain * lrelu(conv + bias) [+ addend].
    ``filters``: a PreparedFilters that may hold this layer's transformed filter (the per-call transform is then skipped)."""
    _chk(x, 'x'); _chk(wp, 'wp'); _chk(bias, 'bias'); _chk(addend, 'addend')
    N, H, W, C = x.shape
    Ho, Wo = out_size(H, KH, stride, pad), out_size(W, KW, stride, pad)
    if out is None:
        out = torch.empty((N, Ho, Wo, K), device=x.device, dtype=torch.float32)
    _chk(out, 'out')
    d = make_desc(N, H, W, C, K, KH, KW, stride, pad, _ld(x), _ld(out), wp.stride(0))
    nbytes = lib().raw('contrad_conv2d_fwd_workspace_bytes')(ctypes.byref(d))
    ws = _workspace(nbytes, x.device) if nbytes > 0 else None
    if addend is not None and (tuple(addend.shape) != tuple(out.shape) or _ld(addend) != _ld(out)):
        raise RuntimeError('contrad_hip: addend must match y in shape and leading dimension')
    u = filters.get(0, wp) if filters is not None else None
    if u is not None:
        _conv_call(0, d, 'contrad_conv2d_fwd_add_u', ctypes.byref(d), _p(x), _p(wp), _p(bias), _p(addend), _p(out),
                   float(slope), float(gain), _p(ws), nbytes, ctypes.byref(u), _stream())
        return out
    _conv_call(0, d, 'contrad_conv2d_fwd_add', ctypes.byref(d), _p(x), _p(wp), _p(bias), _p(addend), _p(out),
               float(slope), float(gain), _p(ws), nbytes, _stream())
    return out


def conv2d_dgrad(gy, wp, x_shape, KH, KW, stride, pad, act_ref=None, slope=1.0, gain=1.0, out=None, filters=None):
    """gy: (N,Ho,Wo,K); returns dx (N,H,W,C) for x_shape=(N,H,W,C); optional fused act' of the producer.
    ``filters``: as in conv2d_fwd."""
    _chk(gy, 'gy'); _chk(wp, 'wp'); _chk(act_ref, 'act_ref')
    N, H, W, C = x_shape
    K = gy.shape[3]
    if out is None:
        out = torch.empty((N, H, W, C), device=gy.device, dtype=torch.float32)
    _chk(out, 'out')
    if act_ref is not None and (tuple(act_ref.shape) != tuple(out.shape) or _ld(act_ref) != _ld(out)):
        raise RuntimeError('contrad_hip: act_ref must match dx in shape and leading dimension')
    d = make_desc(N, H, W, C, K, KH, KW, stride, pad, _ld(out), _ld(gy), wp.stride(0))
    if (d.Ho, d.Wo) != (gy.shape[1], gy.shape[2]):
        raise RuntimeError('contrad_hip: gy spatial size does not match the conv geometry')
    nbytes = lib().raw('contrad_conv2d_dgrad_workspace_bytes')(ctypes.byref(d))
    ws = _workspace(nbytes, gy.device) if nbytes > 0 else None
    u = filters.get(1, wp) if filters is not None else None
    if u is not None:
        _conv_call(1, d, 'contrad_conv2d_dgrad_ws_u', ctypes.byref(d), _p(gy), _p(wp), _p(out), _p(act_ref),
                   float(slope), float(gain), _p(ws), nbytes, ctypes.byref(u), _stream())
        return out
    _conv_call(1, d, 'contrad_conv2d_dgrad_ws', ctypes.byref(d), _p(gy), _p(wp), _p(out), _p(act_ref),
               float(slope), float(gain), _p(ws), nbytes, _stream())
    return out


def conv2d_wino(mode, inp, wp, C, K, bias=None, ref=None, slope=1.0, gain=1.0, out=None, k4s2=False, f44=False, k3s2=False):
    """Winograd kernels on ANY shape ``contrad_conv2d_wino_ok`` accepts (conv2d_fwd / conv2d_dgrad pick them by themselves for
    launches that fill the chip).  3x3 stride 1 pad 1 (F(2x2,3x3), csrc/wino.h; ``f44``: F(4x4,3x3), csrc/wino44.h) -- mode 0:
    inp = x (N,H,W,C) -> y (N,H,W,K);
    mode 1: inp = gy (N,H,W,K) -> dx (N,H,W,C) -- or, ``k4s2``, 4x4 stride 2 pad 1 (F(2x2,2x2) on the four phases,
    csrc/wino22.h): mode 0: x (N,H,W,C) -> y (N,H/2,W/2,K); mode 1: gy (N,Ho,Wo,K) -> dx (N,2Ho,2Wo,C) -- or, ``k3s2``, 3x3 stride 2
    pad 0 on an odd map (F(2x2,2x2) on the phases, zero planes skipped, csrc/wino23.h): mode 0 only, x (N,2G+1,2G+1,C) -> y (N,G,G,K).

    Supported 3x3 stride-1 pad-1 shapes (the statement of include/contrad_hip.h and csrc/wino44.h):
      F(2x2,3x3): H and W powers of two >= 4, any aspect ratio; input channels a multiple of 16, output channels of 64.
      F(4x4,3x3): H and W powers of two, either square 4x4 / 8x8 / 16x16, or W >= 32 and H >= 16; input and output channels
                  multiples of 32.
      (Both: input and filter leading dimensions multiples of 4, block-relative offsets below 2^31 bytes.)  ``in`` / ``out``
      are "input" / "output" of the call: x / y in mode 0, gy / dx in mode 1.  Other shapes raise RuntimeError."""
    _chk(inp, 'inp'); _chk(wp, 'wp'); _chk(bias, 'bias'); _chk(ref, 'ref')
    N, Hi, Wi, _ = inp.shape
    co = K if mode == 0 else C
    if k3s2:
        if mode != 0:
            raise RuntimeError('contrad_hip: the 3x3 stride-2 Winograd kernel is forward only')
        H, W = Hi, Wi
        oshape = (N, (H - 1) // 2, (W - 1) // 2, co)
        geo = (3, 3, 2, 0)
    elif k4s2:
        H, W = (Hi, Wi) if mode == 0 else (2 * Hi, 2 * Wi)          # the conv's input map
        oshape = (N, H // 2, W // 2, co) if mode == 0 else (N, H, W, co)
        geo = (4, 4, 2, 1)
    else:
        H, W = Hi, Wi
        oshape = (N, H, W, co)
        geo = (3, 3, 1, 1)
    if out is None:
        out = torch.empty(oshape, device=inp.device, dtype=torch.float32)
    _chk(out, 'out')
    if ref is not None and (tuple(ref.shape) != tuple(out.shape) or _ld(ref) != _ld(out)):
        raise RuntimeError('contrad_hip: ref must match the output in shape and leading dimension')
    d = make_desc(N, H, W, C, K, geo[0], geo[1], geo[2], geo[3], _ld(inp) if mode == 0 else _ld(out),
                  _ld(out) if mode == 0 else _ld(inp), wp.stride(0))
    if f44:
        if k4s2 or lib().raw('contrad_conv2d_wino44_ok')(ctypes.byref(d), mode) != 1:
            raise RuntimeError('contrad_hip: shape not supported by the F(4x4, 3x3) Winograd kernel')
        nbytes = lib().raw('contrad_conv2d_wino44_workspace_bytes')(ctypes.byref(d))
    else:
        if lib().raw('contrad_conv2d_wino_ok')(ctypes.byref(d), mode) != 1:
            raise RuntimeError('contrad_hip: shape not supported by the Winograd kernels')
        nbytes = lib().raw('contrad_conv2d_wino_workspace_bytes')(ctypes.byref(d), mode)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: the Winograd workspace query rejected the shape (%d)' % nbytes)
    ws = _workspace(nbytes, inp.device)
    lib().call('contrad_conv2d_wino44' if f44 else 'contrad_conv2d_wino', ctypes.byref(d), mode, _p(inp), _p(wp), _p(bias), _p(ref), _p(out),
               float(slope), float(gain), _p(ws), ctypes.c_longlong(nbytes), _stream())
    return out


def conv2d_wino_wgrad(x, gy, ldw=None, out=None, dbias=None):
    """Weight gradient of a 3x3 stride-1 pad-1 layer (gy as large as x: F(3x3, 2x2), csrc/wino.h) or of a 4x4 stride-2 pad-1
    layer (gy half as large: F(2x2, 2x2) per input phase, csrc/wino22.h) on the Winograd kernels (forced; conv2d_wgrad picks
    them by itself when the launch fills the chip).  Returns dwp packed (KH * KW * C, ldw)."""
    _chk(x, 'x'); _chk(gy, 'gy')
    N, H, W, C = x.shape
    K = gy.shape[3]
    k, st = (3, 1) if gy.shape[1] == H else (4, 2)
    if out is None:
        out = torch.zeros((k * k * C, ldw or round_up(K, 4)), device=x.device, dtype=torch.float32)
    _chk(out, 'out')
    d = make_desc(N, H, W, C, K, k, k, st, 1, _ld(x), _ld(gy), out.stride(0))
    if lib().raw('contrad_conv2d_wino_ok')(ctypes.byref(d), 2) != 1:
        raise RuntimeError('contrad_hip: shape not supported by the Winograd weight-gradient kernel')
    nbytes = lib().raw('contrad_conv2d_wino_workspace_bytes')(ctypes.byref(d), 2)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: the Winograd workspace query rejected the shape (%d)' % nbytes)
    ws = _workspace(nbytes, x.device)
    lib().call('contrad_conv2d_wino_wgrad', ctypes.byref(d), _p(x), _p(gy), _p(out), _p(dbias), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


_ws_cache = {}


class private_workspace(object):
    """Scratch buffers allocated inside this scope belong to ``owner_dict`` (held by the caller) instead of the
    process-wide cache.  A captured hipGraph bakes raw scratch pointers into its nodes, and every ``torch.cuda.graph``
    capture runs on the same capture stream: without this, a second captured graph would reuse -- or, when it needs
    more, REPLACE and thereby free -- the buffer the first graph still writes to.  Each Graphed*Step wraps its capture
    in one of these and keeps ``owner_dict`` alive as long as its graph."""

    def __init__(self, owner_dict):
        self.mine = owner_dict

    def __enter__(self):
        global _ws_cache
        self.saved, _ws_cache = _ws_cache, self.mine
        return self

    def __exit__(self, *exc):
        global _ws_cache
        _ws_cache = self.saved
        return False


def _workspace(nbytes, device):
    """Grow-only per-device scratch (reused across calls on the same stream; torch owns the memory)."""
    key = (device.index, _stream_handle())
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() * 4 < nbytes:
        buf = torch.empty((max(nbytes, 1) + 3) // 4, device=device, dtype=torch.float32)
        _ws_cache[key] = buf
    return buf


def conv2d_wgrad(x, gy, KH, KW, stride, pad, ldw=None, out=None, dbias=None):
    """Returns dwp packed (KH*KW*C, ldw); optionally also writes the bias gradient sum(gy) into ``dbias`` (K,)."""
    _chk(x, 'x'); _chk(gy, 'gy')
    N, H, W, C = x.shape
    K = gy.shape[3]
    if out is None:
        ldw = ldw or round_up(K, 4)
        out = torch.zeros((KH * KW * C, ldw), device=x.device, dtype=torch.float32)
    _chk(out, 'out')
    d = make_desc(N, H, W, C, K, KH, KW, stride, pad, _ld(x), _ld(gy), out.stride(0))
    nbytes = lib().raw('contrad_conv2d_wgrad_workspace_bytes')(ctypes.byref(d))
    if nbytes < 0:
        raise RuntimeError('contrad_hip: bad conv descriptor (%d)' % nbytes)
    ws = _workspace(nbytes, x.device)
    _conv_call(2, d, 'contrad_conv2d_wgrad', ctypes.byref(d), _p(x), _p(gy), _p(out), _p(dbias), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


# --------------------------------------------------------------------------------------------------
# contrastive losses
# --------------------------------------------------------------------------------------------------
def l2norm_fwd(u):
    _chk(u, 'u')
    R, D = u.shape
    z = torch.empty((R, D), device=u.device, dtype=torch.float32)
    inv = torch.empty((R,), device=u.device, dtype=torch.float32)
    lib().call('contrad_l2norm_fwd', _p(u), _ld(u), _p(z), _p(inv), R, D, 1e-12, _stream())
    return z, inv


def l2norm_bwd(dz, z, inv, out=None, accumulate=False):
    R, D = z.shape
    if out is None:
        out = torch.empty((R, D), device=z.device, dtype=torch.float32)
    lib().call('contrad_l2norm_bwd', _p(dz), _p(z), _p(inv), _p(out), _ld(out), R, D, int(accumulate), _stream())
    return out


def contrast_fwd(z, N, mode, temperature):
    """z (R,D) normalised rows; returns (loss[1], lse[R])."""
    _chk(z, 'z')
    if not z.is_contiguous():
        raise RuntimeError('contrad_hip: z must be contiguous')
    R, D = z.shape
    lse = torch.empty((R,), device=z.device, dtype=torch.float32)
    rowloss = torch.empty((R,), device=z.device, dtype=torch.float32)
    loss = torch.empty((1,), device=z.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_contrast_workspace_bytes')(R, D)
    ws = _workspace(nbytes, z.device)
    lib().call('contrad_contrast_fwd', _p(z), R, D, N, mode, 1.0 / temperature, _p(lse), _p(rowloss), _p(loss),
               _p(ws), nbytes, _stream())
    return loss, lse


def contrast_bwd(z, lse, N, mode, temperature, grad_scale=None):
    R, D = z.shape
    dz = torch.empty((R, D), device=z.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_contrast_workspace_bytes')(R, D)
    ws = _workspace(nbytes, z.device)
    lib().call('contrad_contrast_bwd', _p(z), _p(lse), R, D, N, mode, 1.0 / temperature, _p(grad_scale), _p(dz),
               _p(ws), nbytes, _stream())
    return dz


# The same calls on two independent problems per launch (ContraD: NT-Xent on z1, SupCon on z2); every result is bitwise
# that of the single call.
def l2norm_fwd_pair(u1, u2):
    """-> (z1, inv1, z2, inv2) in one launch."""
    probs = (L2normProblem * 2)()
    outs = []
    for q, u in zip(probs, (u1, u2)):
        _chk(u, 'u')
        R, D = u.shape
        z = torch.empty((R, D), device=u.device, dtype=torch.float32)
        inv = torch.empty((R,), device=u.device, dtype=torch.float32)
        q.u, q.ldu, q.z, q.inv_norm, q.R, q.D = u.data_ptr(), _ld(u), z.data_ptr(), inv.data_ptr(), R, D
        outs += [z, inv]
    lib().call('contrad_l2norm_fwd_batched', probs, 2, 1e-12, _stream())
    return tuple(outs)


def l2norm_bwd_pair(items):
    """items: two of (dz, z, inv, out, zero_rows); rows [R, R + zero_rows) of ``out`` (a view of a taller buffer) get zeros.
    One launch."""
    probs = (L2normProblem * 2)()
    for q, (dz, z, inv, out, zero_rows) in zip(probs, items):
        R, D = z.shape
        q.dz, q.z, q.inv_norm, q.du = dz.data_ptr(), z.data_ptr(), inv.data_ptr(), out.data_ptr()
        q.ldu, q.R, q.D, q.accumulate, q.zero_rows = _ld(out), R, D, 0, int(zero_rows)
    lib().call('contrad_l2norm_bwd_batched', probs, 2, _stream())


def _contrast_pair(items, temperature):
    probs = (ContrastProblem * 2)()
    sizes = []
    for z, N, mode in items:
        _chk(z, 'z')
        if not z.is_contiguous():
            raise RuntimeError('contrad_hip: z must be contiguous')
        sizes.append(round_up(lib().raw('contrad_contrast_workspace_bytes')(z.shape[0], z.shape[1]), 16))
    ws = _workspace(sum(sizes), items[0][0].device)
    off = 0
    for q, (z, N, mode), nb in zip(probs, items, sizes):
        q.z, q.R, q.D, q.N, q.mode, q.inv_temp = z.data_ptr(), z.shape[0], z.shape[1], N, mode, 1.0 / temperature
        q.workspace, q.workspace_bytes = ws.data_ptr() + off, nb
        off += nb
    return probs, ws


def contrast_fwd_pair(z1, N1, mode1, z2, N2, mode2, temperature):
    """-> (loss1, lse1, loss2, lse2): contrast_fwd of both problems in one pair of launches."""
    probs, ws = _contrast_pair(((z1, N1, mode1), (z2, N2, mode2)), temperature)
    outs = []
    for q, z in zip(probs, (z1, z2)):
        R = z.shape[0]
        lse = torch.empty((R,), device=z.device, dtype=torch.float32)
        rowloss = torch.empty((R,), device=z.device, dtype=torch.float32)
        loss = torch.empty((1,), device=z.device, dtype=torch.float32)
        q.lse, q.rowloss, q.loss = lse.data_ptr(), rowloss.data_ptr(), loss.data_ptr()
        outs += [loss, lse, rowloss]
    lib().call('contrad_contrast_fwd_batched', probs, 2, _stream())
    return outs[0], outs[1], outs[3], outs[4]


def contrast_bwd_pair(z1, lse1, N1, mode1, gs1, z2, lse2, N2, mode2, gs2, temperature):
    """-> (dz1, dz2): contrast_bwd of both problems in one pair of launches."""
    probs, ws = _contrast_pair(((z1, N1, mode1), (z2, N2, mode2)), temperature)
    outs = []
    for q, z, lse, gs in zip(probs, (z1, z2), (lse1, lse2), (gs1, gs2)):
        dz = torch.empty(tuple(z.shape), device=z.device, dtype=torch.float32)
        q.lse, q.grad_scale, q.dz = lse.data_ptr(), (gs.data_ptr() if gs is not None else None), dz.data_ptr()
        outs.append(dz)
    lib().call('contrad_contrast_bwd_batched', probs, 2, _stream())
    return outs[0], outs[1]


# --------------------------------------------------------------------------------------------------
# weight preparation (spectral norm / fixed scale + packing), batched
# --------------------------------------------------------------------------------------------------
from ._lib import SnBatch, SnLayer, AdamBatch, SN_MAX_LAYERS, ADAM_MAX_TENSORS, AUG_NPARAM  # noqa: E402


class SnSpec(object):
    """Static description of one layer for the batched weight prep: weight (K, C, KH, KW) [or (K, C) for a
    linear], optional spectral-norm buffers, destination view inside a packed buffer."""
    __slots__ = ('w', 'u', 'v', 'K', 'C', 'T', 'fixed_scale')

    def __init__(self, w, u=None, v=None, fixed_scale=0.0, view_kct=None):
        self.w, self.u, self.v = w, u, v
        if view_kct is not None:
            self.K, self.C, self.T = view_kct
        elif w.dim() == 4:
            self.K, self.C, self.T = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
        else:
            self.K, self.C, self.T = w.shape[0], w.shape[1], 1
        assert self.K * self.C * self.T == w.numel()
        self.fixed_scale = float(fixed_scale)


def sn_scratch_floats(specs):
    offs, tot = [], 0
    for s in specs:
        offs.append(tot)
        tot += int(lib().raw('contrad_sn_scratch_floats')(s.K, s.C, s.T))
        tot = round_up(tot, 4)
    return offs, tot


def _sn_batches(specs, wps, ldws, offs, u_snaps=None, v_snaps=None, gwps=None, gws=None):
    """Yield (SnBatch, first_layer_index) chunks of at most SN_MAX_LAYERS layers."""
    for start in range(0, len(specs), SN_MAX_LAYERS):
        b = SnBatch()
        chunk = specs[start:start + SN_MAX_LAYERS]
        b.n = len(chunk)
        for j, s in enumerate(chunk):
            i = start + j
            L = b.layers[j]
            L.w = s.w.data_ptr()
            L.u = s.u.data_ptr() if s.u is not None else None
            L.v = s.v.data_ptr() if s.v is not None else None
            L.u_snap = u_snaps[i].data_ptr() if (u_snaps is not None and u_snaps[i] is not None) else None
            L.v_snap = v_snaps[i].data_ptr() if (v_snaps is not None and v_snaps[i] is not None) else None
            L.wp = wps[i].data_ptr()
            L.gwp = gwps[i].data_ptr() if gwps is not None else None
            L.gw = gws[i].data_ptr() if gws is not None else None
            L.K, L.C, L.T, L.ldw = s.K, s.C, s.T, ldws[i]
            L.fixed_scale = s.fixed_scale
            b.scratch_off[j] = offs[i]
        yield b, start


def sn_weight_prep(specs, wps, ldws, training, scratch, offs, sigma, u_snaps=None, v_snaps=None, eps=1e-12):
    for b, start in _sn_batches(specs, wps, ldws, offs, u_snaps, v_snaps):
        lib().call('contrad_sn_weight_prep', ctypes.byref(b), int(bool(training)), float(eps), _p(scratch),
                   ctypes.c_void_p(sigma.data_ptr() + 4 * start), _stream())


def sn_weight_grad(specs, wps, ldws, gwps, gws, scratch, offs, sigma, u_snaps=None, v_snaps=None):
    for b, start in _sn_batches(specs, wps, ldws, offs, u_snaps, v_snaps, gwps, gws):
        lib().call('contrad_sn_weight_grad', ctypes.byref(b), _p(scratch),
                   ctypes.c_void_p(sigma.data_ptr() + 4 * start), _stream())


# --------------------------------------------------------------------------------------------------
# RGB-end convolutions
# --------------------------------------------------------------------------------------------------
def rgb_conv_fwd(img, wp, bias, K, k, in_scale, in_shift, slope, gain, out=None):
    """img NCHW (N,3,H,W) -> NHWC (N,H,W,K)."""
    _chk(img, 'img'); _chk(wp, 'wp'); _chk(bias, 'bias')
    if not img.is_contiguous():
        raise RuntimeError('contrad_hip: image batch must be contiguous NCHW')
    N, Cin, H, W = img.shape
    if out is None:
        out = torch.empty((N, H, W, K), device=img.device, dtype=torch.float32)
    lib().call('contrad_rgb_conv_fwd', _p(img), _p(wp), _p(bias), _p(out), N, Cin, H, W, K, k, _ld(out),
               wp.stride(0), float(in_scale), float(in_shift), float(slope), float(gain), _stream())
    return out


def rgb_conv_wgrad(img, gy, k, in_scale, in_shift, dwp, dbias=None):
    _chk(img, 'img'); _chk(gy, 'gy'); _chk(dwp, 'dwp')
    N, Cin, H, W = img.shape
    K = gy.shape[3]
    nbytes = lib().raw('contrad_rgb_conv_wgrad_workspace_bytes')(N, Cin, H, W, K, k)
    ws = _workspace(nbytes, img.device)
    lib().call('contrad_rgb_conv_wgrad', _p(img), _p(gy), _p(dwp), _p(dbias), N, Cin, H, W, K, k, _ld(gy),
               dwp.stride(0), float(in_scale), float(in_shift), _p(ws), ctypes.c_longlong(ws.numel() * 4), _stream())
    return dwp


def rgb_conv_dgrad(gy, wp, bias, C, k, act=0, out_scale=1.0, out_shift=0.0, out=None, mod=None, residual=None):
    """gy NHWC (N,H,W,K) -> NCHW (N,C,H,W), C <= 4; optional per-sample channel modulation (N,K) and NCHW residual."""
    _chk(gy, 'gy'); _chk(wp, 'wp'); _chk(bias, 'bias'); _chk(mod, 'mod'); _chk(residual, 'residual')
    N, H, W, K = gy.shape
    if out is None:
        out = torch.empty((N, C, H, W), device=gy.device, dtype=torch.float32)
    if mod is not None and (tuple(mod.shape) != (N, K) or not mod.is_contiguous()):
        raise RuntimeError('contrad_hip: mod must be a contiguous (N, K) tensor')
    if residual is not None and (tuple(residual.shape) != (N, C, H, W) or not residual.is_contiguous()):
        raise RuntimeError('contrad_hip: residual must be a contiguous (N, C, H, W) tensor')
    lib().call('contrad_rgb_conv_dgrad', _p(gy), _p(wp), _p(bias), _p(mod), _p(residual), _p(out), N, C, H, W, K, k,
               _ld(gy), wp.stride(0), int(act), float(out_scale), float(out_shift), _stream())
    return out


# --------------------------------------------------------------------------------------------------
# statistics / BatchNorm / losses / Adam
# --------------------------------------------------------------------------------------------------
def colstats(x2d, with_sq=False, out=None, accumulate=False):
    """x2d: (M, K) row-major view (row stride = ld).  Returns (1 or 2, K)."""
    _chk(x2d, 'x')
    M, K = x2d.shape
    ld = _ld(x2d)
    if out is None:
        out = torch.empty((2 if with_sq else 1, K), device=x2d.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_colstats_workspace_bytes')(ctypes.c_longlong(M), K, int(with_sq))
    ws = _workspace(nbytes, x2d.device)
    lib().call('contrad_colstats', _p(x2d), ctypes.c_longlong(M), K, ld, int(with_sq), _p(out), int(accumulate),
               _p(ws), ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


def as_rows(t):
    """(N,H,W,C) NHWC dense tensor / view -> (N*H*W, C) strided matrix view (no copy)."""
    N, H, W, C = t.shape
    return t.as_strided((N * H * W, C), (_ld(t), 1), t.storage_offset())


def bn_relu_apply(x2d, y2d, stats, count, gamma, beta, eps=1e-5, perm_hw=1):
    M, K = x2d.shape
    lib().call('contrad_bn_relu_apply', _p(x2d), _p(y2d), ctypes.c_longlong(M), K, _ld(x2d), _ld(y2d), _p(stats),
               float(count), _p(gamma), _p(beta), float(eps), int(perm_hw), _stream())
    return y2d


def bn_relu_apply_eval(x2d, y2d, mean, var, gamma, beta, eps=1e-5, perm_hw=1):
    """Eval-mode BatchNorm + ReLU: ``mean`` (see bn_eval_mean) and ``var`` (the running variance) are used as they are."""
    M, K = x2d.shape
    if mean.numel() != K or var.numel() != K:
        raise RuntimeError('contrad_hip: bn_relu_apply_eval takes one mean and one variance per column')
    lib().call('contrad_bn_relu_apply_eval', _p(x2d), _p(y2d), ctypes.c_longlong(M), K, _ld(x2d), _ld(y2d), _p(mean),
               _p(var), _p(gamma), _p(beta), float(eps), int(perm_hw), _stream())
    return y2d


def bn_eval_mean(bn, conv_bias=None):
    """The mean an eval-mode BatchNorm subtracts from the output of a layer that ran WITHOUT its bias: running_mean -
    conv bias, rounded once per channel (shared by G_SNDCGAN._bn and CDDLSSampler._prep_g)."""
    return bn.running_mean if conv_bias is None else bn.running_mean - conv_bias


def bn_running_update(stats, count, conv_bias, momentum, running_mean, running_var, num_batches_tracked=None):
    K = running_mean.numel()
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        raise RuntimeError('contrad_hip: num_batches_tracked must be an int64 tensor on the device')
    lib().call('contrad_bn_running_update', _p(stats), float(count), K, _p(conv_bias), float(momentum),
               _p(running_mean), _p(running_var), _p(num_batches_tracked), _stream())


def bn_batch_stats(x2d, conv_bias, momentum, running_mean, running_var, num_batches_tracked=None):
    """colstats(x2d, with_sq=True) + bn_running_update(count = rows) in two launches instead of three; returns stats (2, K)."""
    _chk(x2d, 'x')
    M, K = x2d.shape
    if num_batches_tracked is not None and (num_batches_tracked.dtype != torch.int64 or not num_batches_tracked.is_cuda):
        raise RuntimeError('contrad_hip: num_batches_tracked must be an int64 tensor on the device')
    out = torch.empty((2, K), device=x2d.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_colstats_workspace_bytes')(ctypes.c_longlong(M), K, 1)
    ws = _workspace(nbytes, x2d.device)
    lib().call('contrad_bn_batch_stats', _p(x2d), ctypes.c_longlong(M), K, _ld(x2d), _p(out), _p(conv_bias),
               float(momentum), _p(running_mean), _p(running_var), _p(num_batches_tracked), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


GAN_LOSS_KINDS = {'nonsat': 0, 'wgan': 1, 'hinge': 2, 'lsgan': 3}


def gan_d_loss(logits, N, kind):
    """logits (3N,1) -> (out3 = [loss, mean d_real, mean d_gen], grad (3N,1))."""
    _chk(logits, 'logits')
    out = torch.empty(3, device=logits.device, dtype=torch.float32)
    grad = torch.empty((3 * N, 1), device=logits.device, dtype=torch.float32)
    lib().call('contrad_gan_d_loss', _p(logits), logits.stride(0), N, GAN_LOSS_KINDS[kind], _p(out), _p(grad), _stream())
    return out, grad


def gan_g_loss(logits, kind):
    _chk(logits, 'logits')
    N = logits.shape[0]
    out = torch.empty(1, device=logits.device, dtype=torch.float32)
    grad = torch.empty((N, 1), device=logits.device, dtype=torch.float32)
    lib().call('contrad_gan_g_loss', _p(logits), logits.stride(0), N, GAN_LOSS_KINDS.get(kind, 1), _p(out), _p(grad),
               _stream())
    return out, grad


def adam_step(params, grads, exp_avgs, exp_avg_sqs, step, lr, beta1, beta2, eps=1e-8, grad_scale=1.0):
    n = len(params)
    for start in range(0, n, ADAM_MAX_TENSORS):
        b = AdamBatch()
        m = min(ADAM_MAX_TENSORS, n - start)
        b.n = m
        for j in range(m):
            p, g = params[start + j], grads[start + j]
            if not (p.is_contiguous() and g.is_contiguous()):
                raise RuntimeError('contrad_hip: Adam needs contiguous parameters and gradients')
            t = b.t[j]
            t.p, t.g = p.data_ptr(), g.data_ptr()
            t.m, t.v = exp_avgs[start + j].data_ptr(), exp_avg_sqs[start + j].data_ptr()
            t.numel = p.numel()
        lib().call('contrad_adam_step', ctypes.byref(b), int(step), float(lr), float(beta1), float(beta2),
                   float(eps), float(grad_scale), _stream())


def adam_step_dev(params, grads, exp_avgs, exp_avg_sqs, hyper, beta1, beta2, eps=1e-8):
    """adam_step with {lr / bc1, 1 / sqrt(bc2), grad_scale} taken from the device tensor ``hyper`` (3 floats)."""
    n = len(params)
    for start in range(0, n, ADAM_MAX_TENSORS):
        b = AdamBatch()
        m = min(ADAM_MAX_TENSORS, n - start)
        b.n = m
        for j in range(m):
            p, g = params[start + j], grads[start + j]
            if not (p.is_contiguous() and g.is_contiguous()):
                raise RuntimeError('contrad_hip: Adam needs contiguous parameters and gradients')
            t = b.t[j]
            t.p, t.g = p.data_ptr(), g.data_ptr()
            t.m, t.v = exp_avgs[start + j].data_ptr(), exp_avg_sqs[start + j].data_ptr()
            t.numel = p.numel()
        lib().call('contrad_adam_step_dev', ctypes.byref(b), _p(hyper), float(beta1), float(beta2), float(eps), _stream())


def axpby_(y, x, a, b):
    lib().call('contrad_axpby', _p(y), _p(x), ctypes.c_longlong(y.numel()), float(a), float(b), _stream())
    torch.autograd.graph.increment_version(y)          # raw-pointer write: keep ``_version``-keyed caches honest
    return y


# --------------------------------------------------------------------------------------------------
# augmentation
# --------------------------------------------------------------------------------------------------
def _chk_out(out, like, name):
    """A caller-provided output buffer: same shape, fp32, on the device, dense (the kernels write it with flat indices)."""
    _chk(out, 'out')
    if tuple(out.shape) != tuple(like.shape) or not out.is_contiguous() or out.device != like.device:
        raise RuntimeError('contrad_hip: %s: out must be a contiguous tensor of shape %s on %s' % (name, tuple(like.shape), like.device))


def simclr_augment(x, params, contrast_first, has_contrast, out=None):
    """x NCHW (B,3,H,W); params (B, AUG_NPARAM) on the same device."""
    _chk(x, 'x'); _chk(params, 'params')
    if not x.is_contiguous() or tuple(params.shape) != (x.shape[0], AUG_NPARAM) or not params.is_contiguous():
        raise RuntimeError('contrad_hip: simclr_augment needs contiguous NCHW input and (B,%d) params' % AUG_NPARAM)
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError('contrad_hip: simclr_augment is defined for RGB images')
    if out is None:
        out = torch.empty_like(x)
    _chk_out(out, x, 'simclr_augment')
    nbytes = lib().raw('contrad_simclr_workspace_bytes')(B, H, W)
    ws = _workspace(nbytes, x.device)
    lib().call('contrad_simclr_augment', _p(x), _p(out), _p(params), B, H, W, int(contrast_first), int(has_contrast),
               _p(ws), ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


def gaussian_blur_masked(x, params, kernel1d, radius, out=None):
    _chk(x, 'x'); _chk(params, 'params'); _chk(kernel1d, 'kernel1d')
    if not x.is_contiguous():
        raise RuntimeError('contrad_hip: gaussian_blur_masked needs a contiguous NCHW input')
    B, C, H, W = x.shape
    tmp = torch.empty_like(x)
    if out is None:
        out = torch.empty_like(x)
    _chk_out(out, x, 'gaussian_blur_masked')
    lib().call('contrad_gaussian_blur_masked', _p(x), _p(tmp), _p(out), _p(params), _p(kernel1d), B, H, W,
               int(radius), _stream())
    return out


# --------------------------------------------------------------------------------------------------
# the reference's native StyleGAN2 ops
# --------------------------------------------------------------------------------------------------
def upfirdn2d(x, kernel, up=1, down=1, pad=(0, 0, 0, 0)):
    """x NHWC (B,H,W,C) contiguous, kernel (kh,kw); pad = (x0, x1, y0, y1).  Returns NHWC."""
    _chk(x, 'x'); _chk(kernel, 'kernel')
    if not x.is_contiguous() or not kernel.is_contiguous():
        raise RuntimeError('contrad_hip: upfirdn2d needs contiguous tensors')
    B, H, W, C = x.shape
    kh, kw = kernel.shape
    px0, px1, py0, py1 = pad
    oh = (H * up + py0 + py1 - kh) // down + 1
    ow = (W * up + px0 + px1 - kw) // down + 1
    out = torch.empty((B, oh, ow, C), device=x.device, dtype=torch.float32)
    lib().call('contrad_upfirdn2d', _p(x), _p(kernel), _p(out), B, H, W, C, kh, kw, up, up, down, down,
               px0, px1, py0, py1, _stream())
    return out


def upfirdn2d_fused(x, kernel, up=1, down=1, pad=(0, 0, 0, 0), addend=None, act_ref=None, slope=1.0, gain=1.0,
                    want_out=True, want_out2=False):
    """upfirdn2d with the fused epilogue: v = upfirdn2d(x) [+ addend]; returns (v or None, v * act'(act_ref) or None)."""
    _chk(x, 'x'); _chk(kernel, 'kernel'); _chk(addend, 'addend'); _chk(act_ref, 'act_ref')
    B, H, W, C = x.shape
    kh, kw = kernel.shape
    px0, px1, py0, py1 = pad
    oh = (H * up + py0 + py1 - kh) // down + 1
    ow = (W * up + px0 + px1 - kw) // down + 1
    shape = (B, oh, ow, C)
    for t, nm in ((addend, 'addend'), (act_ref, 'act_ref')):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise RuntimeError('contrad_hip: upfirdn2d_fused %s must be a contiguous tensor of the output shape' % nm)
    if not x.is_contiguous() or not kernel.is_contiguous() or (want_out2 and act_ref is None):
        raise RuntimeError('contrad_hip: upfirdn2d_fused needs contiguous tensors (and act_ref for the second output)')
    out = torch.empty(shape, device=x.device, dtype=torch.float32) if want_out else None
    out2 = torch.empty(shape, device=x.device, dtype=torch.float32) if want_out2 else None
    lib().call('contrad_upfirdn2d_fused', _p(x), _p(kernel), _p(out), B, H, W, C, kh, kw, up, up, down, down,
               px0, px1, py0, py1, _p(addend), _p(act_ref), float(slope), float(gain), _p(out2), _stream())
    return out, out2


def fused_bias_act(x, bias, ref, act, grad, alpha, scale, channels_last_size=None, out=None):
    """Elementwise on a contiguous tensor whose LAST dim is the channel (NHWC / (M,K)).  ``out``: a contiguous tensor of
    x's size that is not x (static-buffer callers)."""
    _chk(x, 'x'); _chk(bias, 'bias'); _chk(ref, 'ref'); _chk(out, 'out')
    if not x.is_contiguous() or (ref is not None and not ref.is_contiguous()):
        raise RuntimeError('contrad_hip: fused_bias_act needs contiguous tensors')
    if out is not None and (not out.is_contiguous() or out.numel() != x.numel() or out.data_ptr() == x.data_ptr()):
        raise RuntimeError('contrad_hip: fused_bias_act writes a contiguous tensor of x\'s size other than x')
    y = torch.empty_like(x) if out is None else out
    C = x.shape[-1]
    lib().call('contrad_fused_bias_act', _p(x), _p(bias), _p(ref), _p(y), ctypes.c_longlong(x.numel()), 1, C,
               int(act), int(grad), float(alpha), float(scale), _stream())
    return y


def lincomb(x, z, a, b):
    if not (x.is_contiguous() and z.is_contiguous()) or x.shape != z.shape:
        raise RuntimeError('contrad_hip: lincomb needs equal-shape contiguous tensors')
    y = torch.empty_like(x)
    lib().call('contrad_lincomb', _p(x), _p(z), _p(y), ctypes.c_longlong(x.numel()), float(a), float(b), _stream())
    return y


def minibatch_stddev(mode, x, gy=None, h=None, cpad=None, splits=None):
    """contrad_minibatch_stddev (stylegan2/discriminator.py:22-33 and its two backward passes) on NHWC x (B,H,W,C).
    mode 0 -> y (B,H,W,Cp); mode 1 (gy (B,H,W,Cp)) -> gx (B,H,W,C); mode 2 (gy, h (B,H,W,C)) -> (gx2, ggy).
    ``splits``: sizes of consecutive sub-batches whose statistics stay separate (several discriminator calls merged into
    one pass, ResidualDiscriminatorP.call_batches): one launch per sub-batch into slices of the same output."""
    _chk(x, 'x')
    B, H, W, C = x.shape
    if not x.is_contiguous():
        raise RuntimeError('contrad_hip: minibatch_stddev needs a dense NHWC input')
    Cp = cpad if gy is None else gy.shape[3]
    out2 = None
    if mode == 0:
        out = torch.empty((B, H, W, Cp), device=x.device, dtype=torch.float32)
    else:
        if not gy.is_contiguous() or tuple(gy.shape[:3]) != (B, H, W):
            raise RuntimeError('contrad_hip: minibatch_stddev needs a dense gy of the output shape')
        out = torch.empty_like(x)
        if mode == 2:
            if not h.is_contiguous() or h.shape != x.shape:
                raise RuntimeError('contrad_hip: minibatch_stddev needs a dense h of the input shape')
            out2 = torch.empty_like(gy)
    splits = list(splits) if splits else [B]
    if sum(splits) != B:
        raise RuntimeError('contrad_hip: minibatch_stddev: splits must sum to the batch size')
    b0 = 0
    for n in splits:
        sl = slice(b0, b0 + n)
        lib().call('contrad_minibatch_stddev', int(mode), _p(x[sl]), _p(gy[sl]) if gy is not None else None,
                   _p(h[sl]) if h is not None else None, _p(out[sl]), _p(out2[sl]) if out2 is not None else None,
                   n, H * W, C, Cp, _stream())
        b0 += n
    return out if mode != 2 else (out, out2)


def sumsq(x, scale):
    """scale * sum(x^2) as a 0-dim tensor, fixed summation order (contrad_sumsq)."""
    _chk(x, 'x')
    x = x if x.is_contiguous() else x.contiguous()
    n = x.numel()
    out = torch.empty((), device=x.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_sumsq_workspace_bytes')(ctypes.c_longlong(n))
    ws = _workspace(nbytes, x.device)
    lib().call('contrad_sumsq', _p(x), ctypes.c_longlong(n), float(scale), _p(out), _p(ws), ctypes.c_longlong(ws.numel() * 4),
               _stream())
    return out


def scale_dev(x, s, c):
    """x * (c * s) with s a 0-dim device tensor (no host read)."""
    _chk(x, 'x'); _chk(s, 's')
    x = x if x.is_contiguous() else x.contiguous()
    y = torch.empty_like(x)
    lib().call('contrad_scale_dev', _p(x), _p(s), float(c), _p(y), ctypes.c_longlong(x.numel()), _stream())
    return y


def pixelnorm(x):
    _chk(x, 'x')
    x = x.contiguous()
    y = torch.empty_like(x)
    lib().call('contrad_pixelnorm', _p(x), _p(y), x.shape[0], x.shape[1], _stream())
    return y


def nhwc_scale(x, s):
    """x (N,H,W,C) contiguous, s (N,C) -> x * s[:, None, None, :]."""
    _chk(x, 'x'); _chk(s, 's')
    N, H, W, C = x.shape
    y = torch.empty_like(x)
    lib().call('contrad_nhwc_scale', _p(x), _p(s.contiguous()), _p(y), N, ctypes.c_longlong(H * W), C, _stream())
    return y


def modconv_tables(layers):
    """``layers``: list of (w [Cout][Cin][T] contiguous, wp packed view, wsq [Cin][Cout] or None, transposed, scale).
    One launch (per 32 layers) writes every packed shared weight and demodulation table of the generator."""
    from ._lib import ModconvBatch, MODCONV_MAX_LAYERS
    for start in range(0, len(layers), MODCONV_MAX_LAYERS):
        chunk = layers[start:start + MODCONV_MAX_LAYERS]
        b = ModconvBatch()
        b.n = len(chunk)
        for j, (w, wp, wsq, transposed, scale) in enumerate(chunk):
            _chk(w, 'w'); _chk(wp, 'wp'); _chk(wsq, 'wsq')
            if not w.is_contiguous() or wp.stride(1) != 1 or (wsq is not None and not wsq.is_contiguous()):
                raise RuntimeError('contrad_hip: modconv_tables needs a contiguous weight / table and unit-stride packed columns')
            L = b.layers[j]
            L.w, L.wp, L.wsq = w.data_ptr(), wp.data_ptr(), (wsq.data_ptr() if wsq is not None else None)
            L.Cout, L.Cin, L.T = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
            L.ldw, L.transposed, L.scale = wp.stride(0), int(bool(transposed)), float(scale)
        lib().call('contrad_modconv_tables', ctypes.byref(b), _stream())


def modconv_demod(layers, eps=1e-8):
    """``layers``: list of (style [B][Cin] with contiguous rows, wsq [Cin][K], out [B][K]); one launch writes every
    out = rsqrt(style^2 @ wsq + eps)."""
    from ._lib import DemodBatch, MODCONV_MAX_LAYERS
    for start in range(0, len(layers), MODCONV_MAX_LAYERS):
        chunk = layers[start:start + MODCONV_MAX_LAYERS]
        b = DemodBatch()
        b.n, b.B = len(chunk), chunk[0][0].shape[0]
        for j, (st, wsq, out) in enumerate(chunk):
            _chk(st, 'style'); _chk(wsq, 'wsq'); _chk(out, 'out')
            if (st.shape[0] != b.B or not st.is_contiguous() or not wsq.is_contiguous() or not out.is_contiguous()
                    or st.shape[1] != wsq.shape[0] or tuple(out.shape) != (b.B, wsq.shape[1])):
                raise RuntimeError('contrad_hip: modconv_demod needs contiguous [B][Cin] / [Cin][K] / [B][K] tensors')
            L = b.layers[j]
            L.style, L.wsq, L.out = st.data_ptr(), wsq.data_ptr(), out.data_ptr()
            L.Cin, L.K = wsq.shape[0], wsq.shape[1]
        lib().call('contrad_modconv_demod', ctypes.byref(b), float(eps), _stream())


def modconv_epilogue_(x, demod, noise, noise_w, bias, out=None, post_scale=None):
    """sqrt2 * lrelu_0.2(x * demod + noise_w * noise + bias) [* post_scale[n,k]] on x (N,H,W,K); in place unless ``out``
    is given.  ``post_scale``: the consuming layer's style vector (its nhwc_scale pass folded into this store)."""
    N, H, W, K = x.shape
    out = x if out is None else out
    lib().call('contrad_modconv_epilogue', _p(x), _p(demod), _p(noise), _p(noise_w), _p(bias), _p(post_scale), _p(out), N,
               ctypes.c_longlong(H * W), K, _stream())
    return out


def upfirdn2d_modconv(x, kernel, pad, demod, noise, noise_w, bias, post_scale=None):
    """Blur (4x4 FIR, up = down = 1, pad = (x0, x1, y0, y1)) followed by modconv_epilogue_ in ONE launch: the tail of the
    generator's upsampling StyledConv (generator.py:80-83,97-118).  x (N,H,W,K) NHWC -> (N,H',W',K)."""
    _chk(x, 'x'); _chk(kernel, 'kernel')
    if tuple(kernel.shape) != (4, 4) or not x.is_contiguous():
        raise RuntimeError('contrad_hip: upfirdn2d_modconv needs a dense NHWC input and the 4x4 FIR')
    N, H, W, K = x.shape
    oh, ow = H + pad[2] + pad[3] - 4 + 1, W + pad[0] + pad[1] - 4 + 1
    # the kernel reads demod / post_scale as float4 at [N][K], bias at [K], noise at [N][oh][ow]: wrong sizes read out of bounds
    for t, nm, shape in ((demod, 'demod', (N, K)), (post_scale, 'post_scale', (N, K)), (bias, 'bias', (K,)),
                         (noise, 'noise', (N, 1, oh, ow))):
        if t is None:
            continue
        _chk(t, nm)
        if t.numel() != int(torch.Size(shape).numel()) or not t.is_contiguous():
            raise RuntimeError('contrad_hip: upfirdn2d_modconv: %s must be a contiguous tensor of %s elements' % (nm, shape))
    if K % 4:
        raise RuntimeError('contrad_hip: upfirdn2d_modconv needs a channel count that is a multiple of 4')
    out = torch.empty(N, oh, ow, K, device=x.device, dtype=torch.float32)
    lib().call('contrad_upfirdn2d_modconv', _p(x), _p(kernel), _p(out), N, H, W, K, int(pad[0]), int(pad[1]), int(pad[2]),
               int(pad[3]), _p(demod), _p(noise), _p(noise_w), _p(bias), _p(post_scale), _stream())
    return out


def simclr_augment_bwd(x, params, grad_out, contrast_first, has_contrast):
    B, C, H, W = x.shape
    gin = torch.empty_like(x)
    nbytes = lib().raw('contrad_simclr_augment_bwd_workspace_bytes')(B, H, W)
    ws = _workspace(nbytes, x.device)
    lib().call('contrad_simclr_augment_bwd', _p(x), _p(params), _p(grad_out.contiguous()), _p(gin), B, H, W,
               int(contrast_first), int(has_contrast), _p(ws), ctypes.c_longlong(ws.numel() * 4), _stream())
    return gin


def cutout_masked_(y, params, length):
    """In place on a contiguous NCHW batch: RandomApply(CutOut(length)); also its own backward."""
    _chk(y, 'y'); _chk(params, 'params')
    if not y.is_contiguous():
        raise RuntimeError('contrad_hip: cutout needs a contiguous NCHW batch')
    B, C, H, W = y.shape
    lib().call('contrad_cutout_masked', _p(y), _p(params), B, H, W, int(length), _stream())
    return y


def gaussian_blur_masked_bwd(grad_out, params, kernel1d, radius):
    B, C, H, W = grad_out.shape
    tmp = torch.empty_like(grad_out)
    gin = torch.empty_like(grad_out)
    lib().call('contrad_gaussian_blur_masked_bwd', _p(grad_out.contiguous()), _p(tmp), _p(gin), _p(params),
               _p(kernel1d), B, H, W, int(radius), _stream())
    return gin


def nhwc_dot(a, b, per_channel=True):
    """a (N,H,W,C) contiguous; b (N,H,W,C) [per_channel] or (N,H,W) / (N,1,H,W) -> (N,C) sums over the pixels."""
    _chk(a, 'a'); _chk(b, 'b')
    N, H, W, C = a.shape
    if not (a.is_contiguous() and b.is_contiguous()) or b.numel() != (a.numel() if per_channel else N * H * W):
        raise RuntimeError('contrad_hip: nhwc_dot needs contiguous (N,H,W,C) / (N,H,W) operands')
    out = torch.empty((N, C), device=a.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_nhwc_dot_workspace_bytes')(N, ctypes.c_longlong(H * W), C)
    ws = _workspace(nbytes, a.device)
    lib().call('contrad_nhwc_dot', _p(a), _p(b), _p(out), N, ctypes.c_longlong(H * W), C, int(per_channel), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


def bn_relu_bwd(dy2d, x2d, stats, count, gamma, beta, eps, reduce_fn=None):
    """Returns (dx2d, dgamma, dbeta).  reduce_fn(out2k) -> global count multiplier hook for SyncBN."""
    M, K = x2d.shape
    ld = _ld(x2d)
    if _ld(dy2d) != ld:
        raise RuntimeError('contrad_hip: dy and x must share the leading dimension')
    out = torch.empty((2, K), device=x2d.device, dtype=torch.float32)
    nbytes = lib().raw('contrad_colstats_workspace_bytes')(ctypes.c_longlong(M), K, 1)
    ws = _workspace(nbytes, x2d.device)
    lib().call('contrad_bn_relu_bwd_stats', _p(dy2d), _p(x2d), ctypes.c_longlong(M), K, ld, _p(stats), float(count),
               _p(gamma), _p(beta), float(eps), _p(out), _p(ws), ctypes.c_longlong(ws.numel() * 4), _stream())
    # SyncBN: dx needs the GLOBAL {sum dy, sum dy*xhat}; dgamma / dbeta stay this rank's LOCAL sums (as
    # torch.nn.SyncBatchNorm returns them) -- the gradient exchange averages them like every other parameter
    local = out
    if reduce_fn is not None:
        local = out.clone()
        reduce_fn(out)
    dx = torch.empty_like(x2d)
    if _ld(dx) != ld:
        raise RuntimeError('contrad_hip: bn backward expects dense rows')
    lib().call('contrad_bn_relu_bwd_apply', _p(dy2d), _p(x2d), _p(dx), ctypes.c_longlong(M), K, ld, _p(stats),
               float(count), _p(gamma), _p(beta), float(eps), _p(out), _stream())
    return dx, local[1], local[0]


# ---- linear-evaluation head (csrc/linhead.hip) ----
def linhead_plan(N, K, C):
    """(K-splits, classes per thread of the logits kernel, 64-row tiles) contrad_linhead_fwd takes for (N, K, C)."""
    s, ct, rt = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
    lib().call('contrad_linhead_plan', int(N), int(K), int(C), ctypes.byref(s), ctypes.byref(ct), ctypes.byref(rt))
    return s.value, ct.value, rt.value


def _chk_labels(y, N, C):
    if y.dtype != torch.int64 or y.dim() != 1 or y.numel() != N or not y.is_contiguous():
        raise RuntimeError('contrad_hip: labels must be a contiguous int64 vector of %d entries' % N)
    if not y.is_cuda:           # host labels can be checked before the launch; device labels are handled by the kernel
        if N and (int(y.min()) < 0 or int(y.max()) >= C):
            raise RuntimeError('contrad_hip: label outside [0, %d)' % C)


def linhead_fwd(feats, weight, bias, y=None, dl_scale=None, logits=None, dlogits=None, meters=None, want_logits=True,
                want_dlogits=False):
    """Launches 1 + 2 of the head: logits = feats @ weight.T + bias and, with labels ``y`` (int64; a CPU tensor is
    range-checked here and uploaded), the cross-entropy meters and ``dlogits = (softmax - onehot) * dl_scale``
    (default 1 / N).  ``meters`` (4 float64 on the device: loss sum, top-1 hits, top-5 hits, samples) is added to in
    place.  Returns (logits or None, dlogits or None)."""
    _chk(feats, 'feats'); _chk(weight, 'weight'); _chk(bias, 'bias')
    N, K = feats.shape
    C = weight.shape[0]
    if weight.dim() != 2 or weight.shape[1] != K or not weight.is_contiguous() or not 1 <= C <= 128:
        raise RuntimeError('contrad_hip: weight must be a contiguous (C, %d) matrix with 1 <= C <= 128' % K)
    if bias is not None and (bias.numel() != C or not bias.is_contiguous()):
        raise RuntimeError('contrad_hip: bias must hold %d contiguous floats' % C)
    if y is not None:
        _chk_labels(y, N, C)
        y = y.to(feats.device)
    elif want_dlogits or dlogits is not None or meters is not None:
        raise RuntimeError('contrad_hip: loss, meters and dlogits need labels')
    if meters is not None and (meters.dtype != torch.float64 or not meters.is_cuda or meters.numel() != 4
                               or not meters.is_contiguous()):
        raise RuntimeError('contrad_hip: meters must be 4 contiguous CUDA float64 values')
    if logits is None and want_logits:
        logits = torch.empty(N, C, device=feats.device, dtype=torch.float32)
    if dlogits is None and want_dlogits:
        dlogits = torch.empty(N, C, device=feats.device, dtype=torch.float32)
    for t, nm in ((logits, 'logits'), (dlogits, 'dlogits')):
        _chk(t, nm)
        if t is not None and (tuple(t.shape) != (N, C) or not t.is_contiguous()):
            raise RuntimeError('contrad_hip: %s must be a contiguous (%d, %d) tensor' % (nm, N, C))
    ws = _workspace(lib().raw('contrad_linhead_workspace_bytes')(N, K, C), feats.device)
    lib().call('contrad_linhead_fwd', _p(feats), _ld(feats), _p(weight), _p(bias), _p(y), N, K, C,
               float(1.0 / N if dl_scale is None else dl_scale), _p(logits), _p(dlogits), _p(meters), _p(ws), _stream())
    if meters is not None:
        torch.autograd.graph.increment_version(meters)
    return logits, dlogits


def linhead_wgrad_sgd(feats, dlogits, weight=None, bias=None, lr=None, grad_weight=None, grad_bias=None):
    """Launch 3: gradW = dlogits.T @ feats, gradb = dlogits.sum(0); with ``lr`` (a 1-element CUDA float tensor)
    ``weight`` / ``bias`` take the SGD step in place; ``grad_weight`` / ``grad_bias`` (optional) receive the gradients."""
    _chk(feats, 'feats'); _chk(dlogits, 'dlogits'); _chk(weight, 'weight'); _chk(bias, 'bias'); _chk(lr, 'lr')
    _chk(grad_weight, 'grad_weight'); _chk(grad_bias, 'grad_bias')
    N, K = feats.shape
    C = dlogits.shape[1]
    if tuple(dlogits.shape) != (N, C) or not dlogits.is_contiguous() or not 1 <= C <= 128:
        raise RuntimeError('contrad_hip: dlogits must be a contiguous (%d, C) tensor with 1 <= C <= 128' % N)
    for t, nm, shape in ((weight, 'weight', (C, K)), (grad_weight, 'grad_weight', (C, K)), (bias, 'bias', (C,)),
                         (grad_bias, 'grad_bias', (C,))):
        if t is not None and (tuple(t.shape) != shape or not t.is_contiguous()):
            raise RuntimeError('contrad_hip: %s must be a contiguous %s tensor' % (nm, shape))
    if lr is not None and weight is None:
        raise RuntimeError('contrad_hip: the SGD form needs the weight')
    if lr is None and grad_weight is None and grad_bias is None:
        raise RuntimeError('contrad_hip: nothing to compute (neither lr nor a gradient output)')
    upd = lr is not None
    lib().call('contrad_linhead_wgrad_sgd', _p(feats), _ld(feats), _p(dlogits), N, K, C, _p(lr),
               _p(weight if upd else None), _p(bias if upd else None), _p(grad_weight), _p(grad_bias), _stream())
    if upd:
        torch.autograd.graph.increment_version(weight)
        if bias is not None:
            torch.autograd.graph.increment_version(bias)
    return grad_weight, grad_bias


# ---- similarity-matrix kernels: the checks csrc/knn.hip, prdc.hip and kid.hip share ----
def _chk_S(S, n):
    _chk(S, 'S')
    if S.dim() != 2 or S.shape[0] < 1:
        raise RuntimeError('contrad_hip: S must be a non-empty (M, ldS) matrix')
    if not 1 <= int(n) <= S.shape[1]:
        raise RuntimeError('contrad_hip: n = %d outside [1, %d] (the columns of S)' % (n, S.shape[1]))
    return S.shape[0], _ld(S), int(n)


def _as_int(t):
    return ctypes.cast(_p(t), ctypes.POINTER(ctypes.c_int))                    # (the header's int* maps to a typed pointer)


def _chk_k(k, n, self0, limit):
    """1 <= k <= the shortest row of the launch (n - 1 columns where ``self0`` leaves one out) and the kernel's own
    ``limit`` on k (None: the row alone)."""
    remain = n - 1 if 0 <= self0 < n else n
    top = remain if limit is None else min(remain, limit)
    if not 1 <= k <= top:
        if limit is not None and remain == n:
            raise RuntimeError('contrad_hip: k = %d outside [1, min(n, %d)] with n = %d' % (k, limit, n))
        raise RuntimeError('contrad_hip: k = %d outside [1, %d] (n = %d, self0 = %d)' % (k, top, n, self0))


# ---- weighted kNN vote (csrc/knn.hip) ----
KNN_MAX_K = 1024
KNN_MAX_CLASSES = 1024


def knn_select(S, n, labels, n_classes, k, inv_temp, self0=-1):
    """Per row of the similarity matrix ``S`` (M, ldS >= n; columns [0, n) are read) the k nearest of the n bank
    columns and their weighted class vote.  ``labels``: int64 CUDA vector of the n bank labels.  ``self0``: column
    ``self0 + i`` is left out of row i when it lies in [0, n) (``self0 < 0``: nothing is left out), by index.  Returns
    (idx int32 (M, k), val (M, k), scores (M, n_classes), pred int32 (M,)): contrad_knn_select's contract, with ``self0``
    contrad_knn_select_loo's (include/contrad_hip.h)."""
    M, ldS, n = _chk_S(S, n)
    C, k, self0 = int(n_classes), int(k), int(self0)
    _chk_k(k, n, self0, KNN_MAX_K)
    if not 1 <= C <= KNN_MAX_CLASSES:
        raise RuntimeError('contrad_hip: n_classes = %d outside [1, %d]' % (C, KNN_MAX_CLASSES))
    if not torch.is_tensor(labels) or not labels.is_cuda:
        raise RuntimeError('contrad_hip: labels must be a CUDA int64 tensor')
    _chk_labels(labels, n, C)
    dev = S.device
    idx = torch.empty((M, k), device=dev, dtype=torch.int32)
    val = torch.empty((M, k), device=dev, dtype=torch.float32)
    scores = torch.empty((M, C), device=dev, dtype=torch.float32)
    pred = torch.empty((M,), device=dev, dtype=torch.int32)
    nbytes = lib().raw('contrad_knn_select_workspace_bytes')(M, n, k, C)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: bad kNN shape (%d)' % nbytes)
    ws = _workspace(nbytes, dev) if nbytes > 0 else None
    lib().call('contrad_knn_select_loo', _p(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(self0), _p(labels), C, k,
               float(inv_temp), _as_int(idx), _p(val), _p(scores), _as_int(pred), _p(ws), ctypes.c_longlong(nbytes), _stream())
    return idx, val, scores, pred


# ---- precision / recall / density / coverage (csrc/prdc.hip) ----
def _chk_vec(t, name, numel, dtype):
    if t is None:
        return
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or t.dim() != 1 or t.numel() != numel \
            or not t.is_contiguous():
        raise RuntimeError('contrad_hip: %s must be a contiguous CUDA %s vector of %d elements'
                           % (name, str(dtype).replace('torch.', ''), numel))


def prdc_kth(S, n, k, self0=-1, out=None):
    """thr (M,): per row of ``S`` (M, ldS >= n; columns [0, n) are read) the k-th largest value, column ``self0 + i`` left
    out of row i when it lies in [0, n) (``self0 < 0``: nothing is left out).  ``out``: a float32 CUDA vector of M elements
    to write into.  contrad_prdc_kth's contract (include/contrad_hip.h)."""
    M, ldS, n = _chk_S(S, n)
    k, self0 = int(k), int(self0)
    _chk_k(k, n, self0, None)
    if out is None:
        out = torch.empty((M,), device=S.device, dtype=torch.float32)
    _chk_vec(out, 'out', M, torch.float32)
    lib().call('contrad_prdc_kth', _p(S), ctypes.c_longlong(ldS), M, n, k, ctypes.c_longlong(self0), _p(out), _stream())
    return out


def prdc_count(S, n, thr_row=None, thr_col=None, row_hits=None, col_hits_c=None, col_hits_r=None):
    """One pass over ``S`` (M, ldS >= n): with ``thr_col`` (n,) ``row_hits`` (M,) int32 is WRITTEN (a new vector unless given)
    and ``col_hits_c`` (n,) int32 ADDED to; with ``thr_row`` (M,) ``col_hits_r`` (n,) int32 is ADDED to.  The column arrays
    are the caller's (zeroed once, one call per row chunk).  Returns ``row_hits`` (None without ``thr_col``).
    contrad_prdc_count's contract (include/contrad_hip.h)."""
    M, ldS, n = _chk_S(S, n)
    if thr_row is None and thr_col is None:
        raise RuntimeError('contrad_hip: prdc_count needs thr_row or thr_col')
    _chk_vec(thr_row, 'thr_row', M, torch.float32); _chk_vec(thr_col, 'thr_col', n, torch.float32)
    if thr_col is not None:
        if col_hits_c is None:
            raise RuntimeError('contrad_hip: thr_col adds into col_hits_c')
        if row_hits is None:
            row_hits = torch.empty((M,), device=S.device, dtype=torch.int32)
    else:
        row_hits = None
    if thr_row is not None and col_hits_r is None:
        raise RuntimeError('contrad_hip: thr_row adds into col_hits_r')
    _chk_vec(row_hits, 'row_hits', M, torch.int32); _chk_vec(col_hits_c, 'col_hits_c', n, torch.int32)
    _chk_vec(col_hits_r, 'col_hits_r', n, torch.int32)
    lib().call('contrad_prdc_count', _p(S), ctypes.c_longlong(ldS), M, n, _p(thr_row), _p(thr_col), _as_int(row_hits),
               _as_int(col_hits_c if thr_col is not None else None), _as_int(col_hits_r if thr_row is not None else None),
               _stream())
    return row_hits


# ---- kernel distance (csrc/kid.hip) ----
MMD_KINDS = {'poly3': 0, 'rq': 1}                                           # contrad_mmd_sums's `kind`


def _sums(who, S, n, kind, self0, gamma, coef0, out, accumulate, T=None):
    """The one body of ``kid_sums``, ``mmd_sums``, ``dot_sums`` and ``gauss_sums``; ``who`` names the caller in the messages
    and its entry point, contrad_<who> (contrad_kid_sums is the kind = 0 entry point and takes no ``kind``; contrad_dot_sums
    takes the second operand ``T`` and neither ``self0``, ``kind``, gamma nor coef0; contrad_gauss_sums takes its ``t`` where
    gamma stands and neither ``kind`` nor coef0)."""
    M, ldS, n = _chk_S(S, n)
    if T is not None:
        _chk(T, 'B')
        if T.dim() != 2 or T.shape[0] != M or T.shape[1] < n or T.device != S.device:
            raise RuntimeError('contrad_hip: %s operands of %s and %s for n = %d (the same rows, at least n columns, one device)'
                               % (who, tuple(S.shape), tuple(T.shape), n))
    elif kind not in MMD_KINDS and kind not in MMD_KINDS.values():
        raise RuntimeError('contrad_hip: %s kind %r (one of %s)' % (who, kind, ', '.join(MMD_KINDS)))
    kind = MMD_KINDS.get(kind, kind)
    gamma, coef0 = float(gamma), float(coef0)
    if not (math.isfinite(gamma) and math.isfinite(coef0)):
        raise RuntimeError('contrad_hip: %s needs a finite gamma and coef0, got %r, %r' % (who, gamma, coef0))
    if out is None:
        if accumulate:
            raise RuntimeError('contrad_hip: %s with accumulate adds to `out`' % who)
        out = torch.empty((1,), device=S.device, dtype=torch.float64)
    _chk_vec(out, 'out', 1, torch.float64)
    if out.device != S.device:
        raise RuntimeError('contrad_hip: out is on %s, S on %s' % (out.device, S.device))
    nbytes = lib().raw('contrad_kid_sums_workspace_bytes')(M, n)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: bad %s shape (%d)' % (who, nbytes))
    ws = _workspace(nbytes, S.device)
    tail = (1 if accumulate else 0, _p(out), _p(ws), ctypes.c_longlong(nbytes), _stream())
    if T is not None:
        lib().call('contrad_' + who, _p(S), ctypes.c_longlong(ldS), _p(T), ctypes.c_longlong(_ld(T)), M, n, *tail)
        return out
    if who == 'gauss_sums':                                                 # t travels in gamma; there is no coef0
        lib().call('contrad_' + who, _p(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(int(self0)), gamma, *tail)
        return out
    kargs = (int(kind),) if who == 'mmd_sums' else ()
    lib().call('contrad_' + who, _p(S), ctypes.c_longlong(ldS), M, n, ctypes.c_longlong(int(self0)), *kargs, gamma, coef0, *tail)
    return out


def kid_sums(S, n, self0=-1, gamma=1.0, coef0=1.0, out=None, accumulate=False):
    """out (1,) float64: the sum over rows i and columns j < n of ``S`` (M, ldS >= n), column ``self0 + i`` left out of row
    i by index (``self0 < 0``: nothing is left out), of (gamma * S[i][j] + coef0)^3, every term in float64.  ``out``: a
    float64 CUDA vector of one element to write into -- or, with ``accumulate``, to add to (a row chunk passes its first
    row as ``self0``).  No atomics: two calls are bitwise equal.  contrad_kid_sums's contract (include/contrad_hip.h)."""
    return _sums('kid_sums', S, n, 0, self0, gamma, coef0, out, accumulate)


def mmd_sums(S, n, kind='poly3', self0=-1, gamma=1.0, coef0=1.0, out=None, accumulate=False):
    """``kid_sums`` with the kernel chosen by ``kind``: 'poly3' (or 0), (gamma * s + coef0)^3, bit for bit ``kid_sums``;
    'rq' (or 1), the rational-quadratic mixture 1 / sqrt(1 + u) + 1 / (1 + u / 2) + 1 / (1 + u / 4)^2 at
    u = max(2 - 2 s, 0) -- S holds similarities of UNIT vectors; gamma and coef0 are not read but must be finite.
    contrad_mmd_sums's contract (include/contrad_hip.h)."""
    return _sums('mmd_sums', S, n, kind, self0, gamma, coef0, out, accumulate)


def dot_sums(A, B, n, out=None, accumulate=False):
    """out (1,) float64: the sum over rows i and columns j < n of ``A[i][j] * B[i][j]`` on ``A`` (M, ldA >= n) and ``B``
    (M, ldB >= n), each product exact in float64, added in ``kid_sums``'s fixed order (no atomics: two calls are bitwise
    equal).  ``B`` may be ``A``: the sum of squares.  ``out`` / ``accumulate``: as in ``kid_sums``.  contrad_dot_sums's
    contract (include/contrad_hip.h)."""
    if B is None:
        raise RuntimeError('contrad_hip: dot_sums needs two operands (pass A twice for the sum of squares)')
    return _sums('dot_sums', A, n, 0, -1, 1.0, 0.0, out, accumulate, T=B)


def gauss_sums(S, n, t=2.0, self0=-1, out=None, accumulate=False):
    """out (1,) float64: the sum over rows i and columns j < n of ``S`` (M, ldS >= n), column ``self0 + i`` left out of row
    i by index, of exp(-t * u) at u = max(2 - 2 S[i][j], 0) -- S holds similarities of UNIT vectors, u is their squared
    distance; every term in float64, added in ``kid_sums``'s fixed order (no atomics: two calls are bitwise equal).
    ``t``: finite and not negative.  ``out`` / ``accumulate``: as in ``kid_sums``.  contrad_gauss_sums's contract
    (include/contrad_hip.h)."""
    t = float(t)
    if not (math.isfinite(t) and t >= 0.0):
        raise RuntimeError('contrad_hip: gauss_sums needs a finite t >= 0, got %r' % (t,))
    return _sums('gauss_sums', S, n, 0, self0, t, 0.0, out, accumulate)


# ---- cDDLS sampling (csrc/cddls.hip) ----
def _flat_f32(t, name):
    _chk(t, name)
    if t is not None and not t.is_contiguous():
        raise RuntimeError('contrad_hip: %s must be contiguous' % name)


def _chk_state(state):
    if state is not None and (state.dtype != torch.int32 or not state.is_cuda or state.numel() < 2
                              or not state.is_contiguous()):
        raise RuntimeError('contrad_hip: the step state must be contiguous CUDA int32 values, at least two: {step, arrival counter = 0}')


def cddls_normal_fill(n, seed, stream_id, step=0, step_dev=None, device=None, want_words=False, out=None, grid_blocks=0):
    """The generator's normals of (seed, stream, step) for elements 0 .. n - 1 -> (normals, raw 32-bit words as int32 or
    None).  ``step_dev`` (int32 device tensor) overrides ``step``; ``grid_blocks`` forces the launch grid."""
    _chk_state(step_dev)
    if out is None:
        out = torch.empty(n, device=device, dtype=torch.float32)
    _flat_f32(out, 'out')
    if out.numel() != n:
        raise RuntimeError('contrad_hip: out must hold %d floats' % n)
    words = torch.empty(n, device=out.device, dtype=torch.int32) if want_words else None
    lib().call('contrad_cddls_normal_fill', _p(out), _p(words), ctypes.c_longlong(n), ctypes.c_longlong(int(seed)),
               int(stream_id), _p(step_dev), int(step), int(grid_blocks), _stream())
    return out, words


def cddls_feature_seed(g_head, c_row, act, slope, out=None):
    """(g_head + c_row) * lrelu'(act) over (N, F) rows; ``out`` may be ``g_head``."""
    _flat_f32(g_head, 'g_head'); _flat_f32(c_row, 'c_row'); _flat_f32(act, 'act')
    F = c_row.numel()
    N = g_head.numel() // F
    if g_head.numel() != N * F or act.numel() != N * F:
        raise RuntimeError('contrad_hip: g_head and act must hold N x %d floats' % F)
    if out is None:
        out = torch.empty_like(g_head)
    _flat_f32(out, 'out')
    if out.numel() != N * F:
        raise RuntimeError('contrad_hip: out must match g_head')
    lib().call('contrad_cddls_feature_seed', _p(g_head), _p(c_row), _p(act), _p(out), ctypes.c_longlong(N), F,
               float(slope), _stream())
    return out


def cddls_pooled_seed(g, c_row, act, slope, out=None):
    """((g + c_row) / T) * lrelu'(act): ``g`` (N, C) is the gradient at a mean over the T pixels of ``act`` (N, ..., C) NHWC;
    ``out`` (act's shape) must not be ``g``."""
    _flat_f32(g, 'g'); _flat_f32(c_row, 'c_row'); _flat_f32(act, 'act')
    C = c_row.numel()
    N = g.numel() // C
    if N < 1 or g.numel() != N * C or act.numel() % (N * C):
        raise RuntimeError('contrad_hip: g must hold N x %d floats and act N x T x %d' % (C, C))
    T = act.numel() // (N * C)
    if out is None:
        out = torch.empty_like(act)
    _flat_f32(out, 'out')
    if out.numel() != act.numel():
        raise RuntimeError('contrad_hip: out must match act')
    lib().call('contrad_cddls_pooled_seed', _p(g), _p(c_row), _p(act), _p(out), ctypes.c_longlong(N), T, C, float(slope),
               _stream())
    return out


def cddls_join_bwd(a, b, act, slope, out=None):
    """(a + b) * lrelu'(act) over equal-size tensors (the backward of a residual join); ``out`` may be ``a``."""
    _flat_f32(a, 'a'); _flat_f32(b, 'b'); _flat_f32(act, 'act')
    if b.numel() != a.numel() or act.numel() != a.numel():
        raise RuntimeError('contrad_hip: a, b and act must have the same size')
    if out is None:
        out = torch.empty_like(a)
    _flat_f32(out, 'out')
    if out.numel() != a.numel():
        raise RuntimeError('contrad_hip: out must match a')
    lib().call('contrad_cddls_join_bwd', _p(a), _p(b), _p(act), _p(out), ctypes.c_longlong(a.numel()), float(slope),
               _stream())
    return out


def bn_relu_bwd_eval(dy2d, y2d, dx2d, gamma, running_var, eps=1e-5, perm_hw=1):
    """Backward of the eval-mode bn_relu_apply(x2d -> y2d): ``dy2d`` in y's layout, ``dx2d`` in x's (may be dy2d when
    perm_hw == 1)."""
    _chk(dy2d, 'dy'); _chk(y2d, 'y'); _chk(dx2d, 'dx'); _chk(gamma, 'gamma'); _chk(running_var, 'running_var')
    M, K = dx2d.shape
    if tuple(dy2d.shape) != (M, K) or tuple(y2d.shape) != (M, K) or _ld(dy2d) != _ld(y2d):
        raise RuntimeError('contrad_hip: dy and y must be (M, K) matrices sharing the leading dimension')
    if gamma.numel() != K or running_var.numel() != K:
        raise RuntimeError('contrad_hip: gamma and running_var must hold K floats')
    lib().call('contrad_cddls_bn_relu_bwd_eval', _p(dy2d), _p(y2d), _p(dx2d), ctypes.c_longlong(M), K, _ld(y2d),
               _ld(dx2d), _p(gamma), _p(running_var), float(eps), int(perm_hw), _stream())
    return dx2d


def cddls_compose(gout, z2, eps, out=None, clamp01=False):
    """gout + eps * z2 (clamped to [0, 1] with ``clamp01``)."""
    _flat_f32(gout, 'gout'); _flat_f32(z2, 'z2')
    if out is None:
        out = torch.empty_like(gout)
    _flat_f32(out, 'out')
    if z2.numel() != gout.numel() or out.numel() != gout.numel():
        raise RuntimeError('contrad_hip: gout, z2 and out must have the same size')
    lib().call('contrad_cddls_compose', _p(gout), _p(z2), _p(out), ctypes.c_longlong(gout.numel()), float(eps),
               int(bool(clamp01)), _stream())
    return out


def cddls_image_end(gx, gout, z2, g_lin, eps, sigma_n, noise=None, seed=0, state=None):
    """Writes ``g_lin`` (gradient at the generator's last pre-activation) and updates ``z2`` in place."""
    for t, nm in ((gx, 'gx'), (gout, 'gout'), (z2, 'z2'), (g_lin, 'g_lin'), (noise, 'noise')):
        _flat_f32(t, nm)
        if t is not None and t.numel() != z2.numel():
            raise RuntimeError('contrad_hip: %s must have the size of z2' % nm)
    _chk_state(state)
    if noise is None and state is None:
        raise RuntimeError('contrad_hip: the generator needs the step state')
    lib().call('contrad_cddls_image_end', _p(gx), _p(gout), _p(z2), _p(g_lin), ctypes.c_longlong(z2.numel()), float(eps),
               float(sigma_n), _p(noise), ctypes.c_longlong(int(seed)), _p(state), _stream())
    torch.autograd.graph.increment_version(z2)


def cddls_latent_update(z, gz, eps, sigma_n, noise=None, seed=0, state=None):
    """z <- clamp(z - eps / 2 * gz + sigma_n sqrt(eps) n, -1, 1) in place; advances ``state[0]``."""
    for t, nm in ((z, 'z'), (gz, 'gz'), (noise, 'noise')):
        _flat_f32(t, nm)
        if t is not None and t.numel() != z.numel():
            raise RuntimeError('contrad_hip: %s must have the size of z' % nm)
    _chk_state(state)
    if noise is None and state is None:
        raise RuntimeError('contrad_hip: the generator needs the step state')
    lib().call('contrad_cddls_latent_update', _p(z), _p(gz), ctypes.c_longlong(z.numel()), float(eps), float(sigma_n),
               _p(noise), ctypes.c_longlong(int(seed)), _p(state), _stream())
    torch.autograd.graph.increment_version(z)


def cddls_energy(d, feat, c_row, bias_term, z2, out=None):
    """Per-sample energy -> (N,): d (N, 1) logits, feat (N, F) in c_row's order, z2 (N, ...)."""
    _chk(d, 'd'); _flat_f32(feat, 'feat'); _flat_f32(c_row, 'c_row'); _flat_f32(bias_term, 'bias_term'); _flat_f32(z2, 'z2')
    N, F = d.shape[0], c_row.numel()
    if feat.numel() != N * F or z2.numel() % N or z2.shape[0] != N:
        raise RuntimeError('contrad_hip: feat must hold N x %d floats and z2 N samples' % F)
    if out is None:
        out = torch.empty(N, device=d.device, dtype=torch.float32)
    _flat_f32(out, 'out')
    if out.numel() != N:
        raise RuntimeError('contrad_hip: out must hold N floats')
    lib().call('contrad_cddls_energy', _p(d), d.stride(0) if N > 1 else 1, _p(feat), _p(c_row), _p(bias_term), _p(z2),
               _p(out), N, F, ctypes.c_longlong(z2.numel() // N), _stream())
    return out


def cddls_recover_loss(gout, target, lambda_feat=0.0, phi=None, phi_target=None, resid=None, out=None):
    """The recovery loss of ``gout`` (N, ...) against ``target`` -> (pix, feat, loss), the rows of ``out`` (3, N).  With
    ``phi`` / ``phi_target`` (N, F) the feature term and its residual rows ``resid`` (N, F) are written too."""
    _flat_f32(gout, 'gout'); _flat_f32(target, 'target')
    N = gout.shape[0]
    if target.numel() != gout.numel() or gout.numel() % N:
        raise RuntimeError('contrad_hip: gout and target must hold the same N samples')
    F = 1
    if phi is not None:
        for t, nm in ((phi, 'phi'), (phi_target, 'phi_target'), (resid, 'resid')):
            if t is None:
                raise RuntimeError('contrad_hip: the feature term needs phi, phi_target and resid')
            _flat_f32(t, nm)
            if t.numel() != phi.numel() or t.numel() % N:
                raise RuntimeError('contrad_hip: %s must hold N feature rows' % nm)
        F = phi.numel() // N
    elif phi_target is not None or resid is not None:
        raise RuntimeError('contrad_hip: phi_target and resid without phi')
    if out is None:
        out = torch.empty(3, N, device=gout.device, dtype=torch.float32)
    _flat_f32(out, 'out')
    if tuple(out.shape) != (3, N):
        raise RuntimeError('contrad_hip: out must be (3, N)')
    lib().call('contrad_cddls_recover_loss', _p(gout), _p(target), _p(phi), _p(phi_target), _p(resid), _p(out[0]),
               _p(out[1]), _p(out[2]), N, F, ctypes.c_longlong(gout.numel() // N), float(lambda_feat), _stream())
    return out[0], out[1], out[2]


def cddls_recover_image_end(gout, target, g_lin, P, gx=None):
    """Writes ``g_lin``: ((2 / P)(gout - target) [+ gx]) through the generator's tanh."""
    for t, nm in ((gout, 'gout'), (target, 'target'), (g_lin, 'g_lin'), (gx, 'gx')):
        _flat_f32(t, nm)
        if t is not None and t.numel() != gout.numel():
            raise RuntimeError('contrad_hip: %s must have the size of gout' % nm)
    lib().call('contrad_cddls_recover_image_end', _p(gx), _p(gout), _p(target), _p(g_lin), ctypes.c_longlong(gout.numel()),
               ctypes.c_longlong(int(P)), _stream())
    return g_lin


def cddls_recover_update(z, gz, m, v, lr, betas, adam_eps, state):
    """One Adam step on ``z`` with the clamp to [-1, 1], ``m`` / ``v`` in place; t = state[0] + 1; advances ``state[0]``."""
    for t, nm in ((z, 'z'), (gz, 'gz'), (m, 'm'), (v, 'v')):
        _flat_f32(t, nm)
        if t.numel() != z.numel():
            raise RuntimeError('contrad_hip: %s must have the size of z' % nm)
    _chk_state(state)
    if state is None:
        raise RuntimeError('contrad_hip: the Adam form needs the step state')
    lib().call('contrad_cddls_recover_update', _p(z), _p(gz), _p(m), _p(v), ctypes.c_longlong(z.numel()), float(lr),
               float(betas[0]), float(betas[1]), float(adam_eps), _p(state), _stream())
    for t in (z, m, v):
        torch.autograd.graph.increment_version(t)


# --------------------------------------------------------------------------------------------------
# baseline training modes (csrc/baseline_aug.hip): hfrt / hflip, DiffAugment, consistency, (2N,1) GAN loss
# --------------------------------------------------------------------------------------------------
HFRT_NPARAM = 4
DIFFAUG_NPARAM = 8
DIFFAUG_STAGES = ('color', 'translation', 'cutout')       # policy bits 1, 2, 4: the order they are applied in


def diffaug_policy_bits(policy):
    """'color,cutout' -> 5.  Stages must come in the order the kernel applies them (the reference's factory order)."""
    names = [p for p in policy.split(',') if p] if isinstance(policy, str) else list(policy)
    idx = [DIFFAUG_STAGES.index(p) if p in DIFFAUG_STAGES else -1 for p in names]
    if not idx or -1 in idx or idx != sorted(set(idx)):
        raise NotImplementedError("DiffAugment policy '%s': a non-empty subset of %s in this order"
                                  % (policy, ','.join(DIFFAUG_STAGES)))
    return sum(1 << i for i in idx)


def _chk_images_params(x, params, nparam, name):
    _chk(x, 'x'); _chk(params, 'params')
    if x.dim() != 4 or not x.is_contiguous() or tuple(params.shape) != (x.shape[0], nparam) or not params.is_contiguous() \
            or params.device != x.device:
        raise RuntimeError('contrad_hip: %s needs contiguous NCHW input and (B,%d) params on its device' % (name, nparam))


def hfrt(x, params, max_pixels, adjoint=False, out=None):
    """HorizontalFlipRandomCrop as an index map (adjoint=True: its transpose on a gradient).  x NCHW (B,C,W,W), params
    (B, HFRT_NPARAM) = {sign, kx, ky, -} on the same device."""
    _chk_images_params(x, params, HFRT_NPARAM, 'hfrt')
    B, C, H, W = x.shape
    if H != W or not 0 <= int(max_pixels) < W:
        raise RuntimeError('contrad_hip: hfrt needs square images and max_pixels < width (got %dx%d, %d)' % (H, W, max_pixels))
    if out is None:
        out = torch.empty_like(x)
    _chk_out(out, x, 'hfrt')
    lib().call('contrad_hfrt', _p(x), _p(out), _p(params), B, C, H, W, int(max_pixels), int(bool(adjoint)), _stream())
    return out


def diffaug(x, params, policy_bits, backward=False, out=None):
    """DiffAugment forward (backward=True: d loss / d x from x = d loss / d y).  x NCHW (B,3,H,W), params (B, DIFFAUG_NPARAM)
    = {b, s, c, tx, ty, ox, oy, -} on the same device."""
    _chk_images_params(x, params, DIFFAUG_NPARAM, 'diffaug')
    B, C, H, W = x.shape
    if C != 3:
        raise RuntimeError('contrad_hip: diffaug is defined for RGB images')
    if not 0 < int(policy_bits) < 8:
        raise RuntimeError('contrad_hip: diffaug policy bits must be in 1..7')
    if out is None:
        out = torch.empty_like(x)
    _chk_out(out, x, 'diffaug')
    nbytes = lib().raw('contrad_diffaug_workspace_bytes')(B, H, W)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: diffaug: unsupported image size %dx%d' % (H, W))
    ws = _workspace(nbytes, x.device)
    lib().call('contrad_diffaug', _p(x), _p(out), _p(params), B, H, W, int(policy_bits), int(bool(backward)), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out


def consistency(a, b, n0, n1, lbd0, lbd1):
    """lbd0 mean_{[0,n0)} (a-b)^2 + lbd1 mean_{[n0,n0+n1)} (a-b)^2 on logit columns a, b (n0+n1, 1) -> (out (1,), grad_a, grad_b)."""
    _chk(a, 'a'); _chk(b, 'b')
    n = int(n0) + int(n1)
    if a.dim() != 2 or b.dim() != 2 or a.shape != (n, 1) or b.shape != (n, 1) or n0 <= 0 or n1 < 0 or a.device != b.device:
        raise RuntimeError('contrad_hip: consistency needs two (%d, 1) logit columns on one device' % n)
    out = torch.empty(1, device=a.device, dtype=torch.float32)
    ga = torch.empty((n, 1), device=a.device, dtype=torch.float32)
    gb = torch.empty((n, 1), device=a.device, dtype=torch.float32)
    lib().call('contrad_consistency', _p(a), max(a.stride(0), 1), _p(b), max(b.stride(0), 1), int(n0), int(n1), float(lbd0),
               float(lbd1), _p(out), _p(ga), _p(gb), _stream())
    return out, ga, gb


def gan_d_loss_2n(logits, N, kind):
    """logits (2N,1), reals first -> (out3 = [loss, mean d_real, mean d_gen], grad (2N,1))."""
    _chk(logits, 'logits')
    if logits.dim() != 2 or tuple(logits.shape) != (2 * N, 1):
        raise RuntimeError('contrad_hip: gan_d_loss_2n needs (2N, 1) logits')
    out = torch.empty(3, device=logits.device, dtype=torch.float32)
    grad = torch.empty((2 * N, 1), device=logits.device, dtype=torch.float32)
    lib().call('contrad_gan_d_loss_2n', _p(logits), max(logits.stride(0), 1), N, GAN_LOSS_KINDS[kind], _p(out), _p(grad),
               _stream())
    return out, grad


# --------------------------------------------------------------------------------------------------
# gradient penalty (csrc/gp.hip): interpolation between two batches, lbd * mean (||grad_n|| - 1)^2 and its cotangent
# --------------------------------------------------------------------------------------------------
def _chk_nchw(t, name, like=None):
    _chk(t, name)
    if t.dim() != 4 or not t.is_contiguous() or t.numel() == 0 or (like is not None and (
            t.shape != like.shape or t.device != like.device)):
        raise RuntimeError('contrad_hip: %s must be a contiguous non-empty NCHW tensor%s' %
                           (name, '' if like is None else ' of shape %s on %s' % (tuple(like.shape), like.device)))


def gp_interpolate(x, g, alpha, out=None):
    """xhat[n] = alpha[n] * x[n] + (1 - alpha[n]) * g[n]; x, g NCHW (N,C,H,W), alpha (N,) on the same device.  Rows with
    alpha 1 / 0 are x / g bit for bit."""
    _chk_nchw(x, 'x'); _chk_nchw(g, 'g', x); _chk(alpha, 'alpha')
    N = x.shape[0]
    if tuple(alpha.shape) != (N,) or not alpha.is_contiguous() or alpha.device != x.device:
        raise RuntimeError('contrad_hip: gp_interpolate needs alpha of shape (%d,) on the images\' device' % N)
    if out is None:
        out = torch.empty_like(x)
    _chk_out(out, x, 'gp_interpolate')
    lib().call('contrad_gp_interpolate', _p(x), _p(g), _p(alpha), _p(out), N, ctypes.c_longlong(x.numel() // N), _stream())
    return out


def gp_penalty(grad, lbd, cot=None):
    """grad NCHW (N,C,H,W) -> (out (1,) = lbd * mean_n (||grad_n||_2 - 1)^2, norms (N,), cot = d out / d grad; cot_n = 0 on a
    zero row)."""
    _chk_nchw(grad, 'grad')
    N = grad.shape[0]
    L = grad.numel() // N
    if cot is None:
        cot = torch.empty_like(grad)
    _chk_out(cot, grad, 'gp_penalty')
    nbytes = lib().raw('contrad_gp_penalty_workspace_bytes')(N, ctypes.c_longlong(L))
    if nbytes < 0:
        raise RuntimeError('contrad_hip: gp_penalty: unsupported size %d x %d' % (N, L))
    ws = _workspace(nbytes, grad.device)
    out = torch.empty(1, device=grad.device, dtype=torch.float32)
    norms = torch.empty(N, device=grad.device, dtype=torch.float32)
    lib().call('contrad_gp_penalty', _p(grad), _p(norms), _p(out), _p(cot), N, ctypes.c_longlong(L), float(lbd), _p(ws),
               ctypes.c_longlong(ws.numel() * 4), _stream())
    return out, norms, cot


# --------------------------------------------------------------------------------------------------
# real-image batches (csrc/data.hip): gather by index, flip, NHWC uint8 -> NCHW float / 255 in one launch
# --------------------------------------------------------------------------------------------------
GATHER_MAX_N = 1 << 24          # the index column of the parameter block is fp32: exact below 2^24


def gather_u8_nchw(src_u8, params, H, W, out=None):
    """out[b, c, i, j] = src_u8[idx_b, i, (flip_b ? W-1-j : j), c] / 255 (bit-equal to ToTensor).  src_u8 uint8 (n, H, W, 3),
    params fp32 (B, 2) rows {index, flip} on the same device; an index outside [0, n) is clamped.  ``out``: a contiguous
    fp32 (B, 3, H, W) tensor to write into (e.g. a captured step's static batch), else a new one."""
    if not torch.is_tensor(src_u8) or not src_u8.is_cuda or src_u8.dtype != torch.uint8:
        raise RuntimeError('contrad_hip: gather_u8_nchw: src must be a CUDA uint8 tensor (got %s, %s)' % (
            getattr(src_u8, 'device', None), getattr(src_u8, 'dtype', type(src_u8))))
    H, W = int(H), int(W)
    if src_u8.dim() != 4 or tuple(src_u8.shape[1:]) != (H, W, 3) or not src_u8.is_contiguous() or src_u8.shape[0] == 0 \
            or H <= 0 or W <= 0:
        raise RuntimeError('contrad_hip: gather_u8_nchw: src must be a contiguous non-empty (n, %d, %d, 3) tensor, got %s' % (
            H, W, tuple(src_u8.shape)))
    n = src_u8.shape[0]
    if n >= GATHER_MAX_N:
        raise NotImplementedError('gather_u8_nchw hands the indices over as floats: fewer than 2^24 images (got %d)' % n)
    _chk(params, 'params')
    if params.dim() != 2 or params.shape[1] != 2 or params.shape[0] == 0 or not params.is_contiguous() \
            or params.device != src_u8.device:
        raise RuntimeError('contrad_hip: gather_u8_nchw: params must be a contiguous non-empty (B, 2) tensor on %s, got %s on %s'
                           % (src_u8.device, tuple(params.shape), params.device))
    B = params.shape[0]
    if out is None:
        out = torch.empty((B, 3, H, W), device=src_u8.device, dtype=torch.float32)
    _chk(out, 'out')
    if tuple(out.shape) != (B, 3, H, W) or not out.is_contiguous() or out.device != src_u8.device:
        raise RuntimeError('contrad_hip: gather_u8_nchw: out must be a contiguous (%d, 3, %d, %d) tensor on %s' % (
            B, H, W, src_u8.device))
    lib().call('contrad_gather_u8_nchw', _p(src_u8), _p(params), _p(out), B, n, H, W, _stream())
    return out


# --------------------------------------------------------------------------------------------------
# images for the host (csrc/imagegrid.hip): float NCHW -> uint8 HWC grid canvas / uint8 NHWC batch in one launch
# --------------------------------------------------------------------------------------------------
def _chk_images(images, who):
    if not torch.is_tensor(images) or not images.is_cuda or images.dtype != torch.float32:
        raise RuntimeError('contrad_hip: %s: images must be a CUDA float32 tensor (got %s, %s)' % (
            who, getattr(images, 'device', None), getattr(images, 'dtype', type(images))))
    if images.dim() != 4 or images.shape[1] != 3 or images.numel() == 0 or not images.is_contiguous():
        raise RuntimeError('contrad_hip: %s: images must be a contiguous non-empty (n, 3, H, W) tensor, got %s with strides %s'
                           % (who, tuple(images.shape), tuple(images.stride())))


def grid_canvas_shape(n, H, W, nrow=8, padding=2):
    """(rows, columns, 3) of make_grid's canvas for n images of H x W: xmaps = min(nrow, n) cells per row."""
    xmaps = min(int(nrow), int(n))
    ymaps = -(-int(n) // xmaps)
    return ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3


def image_grid_u8(images, nrow=8, padding=2, pad_value=0.0, out=None):
    """torchvision's ``make_grid(images, nrow, padding, pad_value=pad_value)`` followed by ``save_image``'s quantisation
    (x * 255 + 0.5, clamped to [0, 255], truncated; NaN -> 0) as ONE launch: fp32 (n, 3, H, W) -> uint8 canvas
    [ymaps * (H + padding) + padding, xmaps * (W + padding) + padding, 3] on the same device.  (A single image is padded
    like any other batch; torchvision returns it unframed.)  ``out``: a contiguous uint8 CUDA tensor of the canvas shape
    with a 4-byte aligned base to write into, else a new one."""
    _chk_images(images, 'image_grid_u8')
    nrow, padding = int(nrow), int(padding)
    if nrow <= 0 or padding < 0:
        raise ValueError('image_grid_u8: nrow > 0 and padding >= 0 expected, got %d, %d' % (nrow, padding))
    n, _, H, W = images.shape
    shape = grid_canvas_shape(n, H, W, nrow, padding)
    if out is None:
        out = torch.empty(shape, device=images.device, dtype=torch.uint8)
    elif not torch.is_tensor(out) or out.dtype != torch.uint8 or out.device != images.device or tuple(out.shape) != shape \
            or not out.is_contiguous() or out.data_ptr() % 4:
        raise RuntimeError('contrad_hip: image_grid_u8: out must be a contiguous 4-byte aligned uint8 %s tensor on %s' % (
            shape, images.device))
    lib().call('contrad_image_grid_u8', _p(images), _p(out), n, H, W, min(nrow, n), padding, float(pad_value), _stream())
    return out


def images_u8(images):
    """fp32 (n, 3, H, W) -> uint8 (n, H, W, 3), quantised as ``hostio.to_uint8``: the grid kernel with one cell per row and
    no padding."""
    _chk_images(images, 'images_u8')
    n, _, H, W = images.shape
    out = torch.empty((n, H, W, 3), device=images.device, dtype=torch.uint8)
    lib().call('contrad_image_grid_u8', _p(images), _p(out), n, H, W, 1, 0, 0.0, _stream())
    return out


# --------------------------------------------------------------------------------------------------
# sliced Wasserstein distance (csrc/eval/swd.hip): pyramid, patch gather, row sort, absolute-difference sum
# --------------------------------------------------------------------------------------------------
def swd_sort_tile():
    """The floats of the row sort's LDS tile (contrad_swd_sort_tile)."""
    return int(lib().raw('contrad_swd_sort_tile')())


def _chk_planes(t, name, who):
    _chk(t, name)
    if t.dim() != 3 or t.shape[1] != t.shape[2] or t.shape[0] < 1 or t.shape[0] % 3 or not t.is_contiguous():
        raise RuntimeError('contrad_hip: %s: %s must be a contiguous (n * 3, R, R) tensor, got %s' % (who, name, tuple(t.shape)))


def swd_u8_planes(x_u8, out=None):
    """uint8 NHWC (n, R, R, 3) -> fp32 planes (n * 3, R, R), plane = image * 3 + channel, the values 0 ... 255 as they are."""
    if not torch.is_tensor(x_u8) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 \
            or x_u8.shape[1] != x_u8.shape[2] or x_u8.shape[0] < 1 or not x_u8.is_contiguous():
        raise RuntimeError('contrad_hip: swd_u8_planes: a contiguous non-empty CUDA uint8 (n, R, R, 3) tensor expected')
    n, R = x_u8.shape[0], x_u8.shape[1]
    if out is None:
        out = torch.empty((n * 3, R, R), device=x_u8.device, dtype=torch.float32)
    _chk_planes(out, 'out', 'swd_u8_planes')
    if tuple(out.shape) != (n * 3, R, R) or out.device != x_u8.device:
        raise RuntimeError('contrad_hip: swd_u8_planes: out must be (%d, %d, %d) on %s' % (n * 3, R, R, x_u8.device))
    lib().call('contrad_swd_u8_planes', _p(x_u8), _p(out), ctypes.c_longlong(n), R, _stream())
    return out


def swd_pyr_down(fine, out=None):
    """One Gaussian pyramid step on planes (P, R, R) -> (P, R / 2, R / 2): the 5 x 5 binomial stencil at the even coordinates,
    mirror boundary.  contrad_swd_pyr_down's contract (include/contrad_hip.h)."""
    _chk_planes(fine, 'fine', 'swd_pyr_down')
    P, R = fine.shape[0], fine.shape[1]
    if R < 4 or R % 2:
        raise RuntimeError('contrad_hip: swd_pyr_down: an even R >= 4 expected, got %d' % R)
    if out is None:
        out = torch.empty((P, R // 2, R // 2), device=fine.device, dtype=torch.float32)
    _chk_planes(out, 'out', 'swd_pyr_down')
    if tuple(out.shape) != (P, R // 2, R // 2) or out.device != fine.device:
        raise RuntimeError('contrad_hip: swd_pyr_down: out must be (%d, %d, %d) on %s' % (P, R // 2, R // 2, fine.device))
    lib().call('contrad_swd_pyr_down', _p(fine), _p(out), ctypes.c_longlong(P), R, _stream())
    return out


def swd_pyr_up_sub(fine, coarse):
    """fine -= up(coarse) in place (planes (P, R, R) and (P, R / 2, R / 2)): the Laplacian step.  Returns ``fine``.
    contrad_swd_pyr_up_sub's contract (include/contrad_hip.h)."""
    _chk_planes(fine, 'fine', 'swd_pyr_up_sub'); _chk_planes(coarse, 'coarse', 'swd_pyr_up_sub')
    P, R = fine.shape[0], fine.shape[1]
    if R < 4 or R % 2 or tuple(coarse.shape) != (P, R // 2, R // 2) or coarse.device != fine.device:
        raise RuntimeError('contrad_hip: swd_pyr_up_sub: fine %s needs an even R >= 4 and coarse (%d, %d, %d) on its device, got %s'
                           % (tuple(fine.shape), P, R // 2, R // 2, tuple(coarse.shape)))
    lib().call('contrad_swd_pyr_up_sub', _p(fine), _p(coarse), ctypes.c_longlong(P), R, _stream())
    return fine


SWD_DESC = 147                                                             # 7 x 7 x 3 values of a descriptor
SWD_BANK_ROWS = 148


def swd_gather(level, cx, cy, nhoods, bank=None, stats=None):
    """The 7 x 7 x 3 patches of ``level`` (planes (n * 3, R, R)) around the centres ``cx``, ``cy`` (int32 CUDA vectors of
    n * nhoods elements, descriptor d in image d // nhoods) as the transposed bank (148, round_up(n * nhoods, 4)) -- row
    c * 49 + dy * 7 + dx, row 147 and the padding columns zero -- and ``stats`` (6,) float64: per channel the sum and the sum
    of squares over all descriptors and positions.  Returns (bank, stats).  contrad_swd_gather's contract."""
    _chk_planes(level, 'level', 'swd_gather')
    n, R, nhoods = level.shape[0] // 3, level.shape[1], int(nhoods)
    if R < 7 or nhoods < 1:
        raise RuntimeError('contrad_hip: swd_gather: R >= 7 and nhoods >= 1 expected, got %d, %d' % (R, nhoods))
    n_desc = n * nhoods
    n_pad = round_up(n_desc, 4)
    _chk_vec(cx, 'cx', n_desc, torch.int32); _chk_vec(cy, 'cy', n_desc, torch.int32)
    if cx is None or cy is None or cx.device != level.device or cy.device != level.device:
        raise RuntimeError('contrad_hip: swd_gather: cx and cy must be int32 vectors on %s' % level.device)
    if bank is None:
        bank = torch.empty((SWD_BANK_ROWS, n_pad), device=level.device, dtype=torch.float32)
    _chk(bank, 'bank')
    if tuple(bank.shape) != (SWD_BANK_ROWS, n_pad) or not bank.is_contiguous() or bank.device != level.device:
        raise RuntimeError('contrad_hip: swd_gather: bank must be a contiguous (%d, %d) tensor on %s' % (SWD_BANK_ROWS, n_pad, level.device))
    if stats is None:
        stats = torch.empty((6,), device=level.device, dtype=torch.float64)
    _chk_vec(stats, 'stats', 6, torch.float64)
    if stats.device != level.device:
        raise RuntimeError('contrad_hip: swd_gather: stats is on %s, the level on %s' % (stats.device, level.device))
    nbytes = lib().raw('contrad_swd_gather_workspace_bytes')(ctypes.c_longlong(n_desc))
    if nbytes < 0:
        raise RuntimeError('contrad_hip: bad swd_gather shape (%d)' % nbytes)
    ws = _workspace(nbytes, level.device)
    lib().call('contrad_swd_gather', _p(level), ctypes.c_longlong(n), R, _as_int(cx), _as_int(cy), nhoods, _p(bank),
               ctypes.c_longlong(n_pad), _p(stats), _p(ws), ctypes.c_longlong(nbytes), _stream())
    return bank, stats


def swd_sort_rows(X, n):
    """Sorts the first ``n`` columns of every row of ``X`` (R, ld >= n) ascending, in place; finite values.  Columns at or
    behind ``n`` are neither read nor written.  Returns ``X``.  contrad_swd_sort_rows's contract (include/contrad_hip.h)."""
    R, ld, n = _chk_S(X, n)
    lib().call('contrad_swd_sort_rows', _p(X), ctypes.c_longlong(ld), R, n, _stream())
    return X


def swd_absdiff_sums(A, B, n, row_offset=None, out=None, accumulate=False):
    """out (1,) float64: the sum over rows r and columns i < n of |A[r][i] - B[r][i] + row_offset[r]| on ``A`` (R, ldA >= n)
    and ``B`` (R, ldB >= n), every term in float64, added in a fixed order (no atomics: two calls are bitwise equal).
    ``row_offset``: a float64 CUDA vector of R elements (None: zero).  ``out`` / ``accumulate``: as in ``kid_sums``.
    contrad_swd_absdiff_sums's contract (include/contrad_hip.h)."""
    R, ldA, n = _chk_S(A, n)
    _chk(B, 'B')
    if B.dim() != 2 or B.shape[0] != R or B.shape[1] < n or B.device != A.device:
        raise RuntimeError('contrad_hip: swd_absdiff_sums operands of %s and %s for n = %d (the same rows, at least n columns, '
                           'one device)' % (tuple(A.shape), tuple(B.shape), n))
    _chk_vec(row_offset, 'row_offset', R, torch.float64)
    if row_offset is not None and row_offset.device != A.device:
        raise RuntimeError('contrad_hip: row_offset is on %s, A on %s' % (row_offset.device, A.device))
    if out is None:
        if accumulate:
            raise RuntimeError('contrad_hip: swd_absdiff_sums with accumulate adds to `out`')
        out = torch.empty((1,), device=A.device, dtype=torch.float64)
    _chk_vec(out, 'out', 1, torch.float64)
    if out.device != A.device:
        raise RuntimeError('contrad_hip: out is on %s, A on %s' % (out.device, A.device))
    nbytes = lib().raw('contrad_swd_absdiff_workspace_bytes')(R, n)
    if nbytes < 0:
        raise RuntimeError('contrad_hip: bad swd_absdiff_sums shape (%d)' % nbytes)
    ws = _workspace(nbytes, A.device)
    lib().call('contrad_swd_absdiff_sums', _p(A), ctypes.c_longlong(ldA), _p(B), ctypes.c_longlong(_ld(B)), _p(row_offset), R, n,
               1 if accumulate else 0, _p(out), _p(ws), ctypes.c_longlong(nbytes), _stream())
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# radial power spectrum (csrc/spectral/spectrum.hip): half-spectrum FFT of the luma, radial bin means, mean 2-D map.  None of
# the three takes scratch: every buffer is an output.

SPEC_SIDES = (16, 32, 64, 128, 256, 512)


def _chk_spec(spec, who):
    """A half spectrum (n, S, S / 2 + 1, 2) -> (n, S)."""
    _chk(spec, 'spec')
    if spec.dim() != 4 or spec.shape[0] < 1 or spec.shape[1] not in SPEC_SIDES or spec.shape[2] != spec.shape[1] // 2 + 1 \
            or spec.shape[3] != 2 or not spec.is_contiguous():
        raise RuntimeError('contrad_hip: %s: spec must be a contiguous (n, S, S / 2 + 1, 2) tensor with S a power of two in '
                           '[16, 512], got %s' % (who, tuple(spec.shape)))
    return int(spec.shape[0]), int(spec.shape[1])


def _chk_dense(t, name, shape, dtype, device, who):
    if not torch.is_tensor(t) or not t.is_cuda or t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous() \
            or t.device != device:
        raise RuntimeError('contrad_hip: %s: %s must be a contiguous %s %s tensor on %s' % (who, name, tuple(shape), dtype, device))


def spec_rfft2(x_u8, twiddles, out=None):
    """The half spectrum (n, S, S / 2 + 1, 2) fp32 of the exact luma (77 R + 150 G + 29 B) / 256 of a uint8 NHWC set
    (n, S, S, 3): numpy.fft.rfft2's layout, real then imaginary part.  ``twiddles``: (S / 2, 2) fp32 on the device,
    (cos, -sin)(2 pi j / S) (``spectrum.twiddles``).  contrad_spec_rfft2's contract (include/contrad_hip.h)."""
    if not torch.is_tensor(x_u8) or not x_u8.is_cuda or x_u8.dtype != torch.uint8 or x_u8.dim() != 4 or x_u8.shape[3] != 3 \
            or x_u8.shape[1] != x_u8.shape[2] or x_u8.shape[0] < 1 or x_u8.shape[1] not in SPEC_SIDES or not x_u8.is_contiguous():
        raise RuntimeError('contrad_hip: spec_rfft2: a contiguous non-empty CUDA uint8 (n, S, S, 3) tensor with S a power of two in '
                           '[16, 512] expected')
    n, S = int(x_u8.shape[0]), int(x_u8.shape[1])
    _chk_dense(twiddles, 'twiddles', (S // 2, 2), torch.float32, x_u8.device, 'spec_rfft2')
    if out is None:
        out = torch.empty((n, S, S // 2 + 1, 2), device=x_u8.device, dtype=torch.float32)
    _chk_dense(out, 'out', (n, S, S // 2 + 1, 2), torch.float32, x_u8.device, 'spec_rfft2')
    lib().call('contrad_spec_rfft2', _p(x_u8), _p(twiddles), _p(out), ctypes.c_longlong(n), S, _stream())
    return out


def spec_radial(spec, bin_of, rcount, out=None):
    """(n, K) float64: the mean of |spec|^2 / S^4 over the full grid's members of every radial bin, from the half spectrum
    with weight 1 in the columns v = 0 and v = S / 2 and 2 elsewhere.  ``bin_of``: (S, S / 2 + 1) int32, ``rcount``: (K,)
    float64 reciprocal member counts (``spectrum.bin_table``), both on the device.  contrad_spec_radial's contract."""
    n, S = _chk_spec(spec, 'spec_radial')
    _chk_dense(bin_of, 'bin_of', (S, S // 2 + 1), torch.int32, spec.device, 'spec_radial')
    if not torch.is_tensor(rcount) or rcount.dim() != 1:
        raise RuntimeError('contrad_hip: spec_radial: rcount must be a (K,) float64 vector')
    K = int(rcount.shape[0])
    _chk_dense(rcount, 'rcount', (K,), torch.float64, spec.device, 'spec_radial')
    if not S // 2 + 1 <= K <= S:
        raise RuntimeError('contrad_hip: spec_radial: %d bins for S = %d (between S / 2 + 1 and S expected)' % (K, S))
    if out is None:
        out = torch.empty((n, K), device=spec.device, dtype=torch.float64)
    _chk_dense(out, 'out', (n, K), torch.float64, spec.device, 'spec_radial')
    lib().call('contrad_spec_radial', _p(spec), _as_int(bin_of), _p(rcount), _p(out), ctypes.c_longlong(n), S, K, _stream())
    return out


def spec_mean_map(spec, out=None, accumulate=False):
    """(S, S / 2 + 1) float64: the sum over the images of |spec|^2 / S^4 (a sum: the caller divides by the number of images
    after the last chunk).  ``accumulate`` adds to ``out``.  contrad_spec_mean_map's contract (include/contrad_hip.h)."""
    n, S = _chk_spec(spec, 'spec_mean_map')
    if out is None:
        if accumulate:
            raise RuntimeError('contrad_hip: spec_mean_map with accumulate adds to `out`')
        out = torch.empty((S, S // 2 + 1), device=spec.device, dtype=torch.float64)
    _chk_dense(out, 'out', (S, S // 2 + 1), torch.float64, spec.device, 'spec_mean_map')
    lib().call('contrad_spec_mean_map', _p(spec), _p(out), ctypes.c_longlong(n), S, 1 if accumulate else 0, _stream())
    return out


# --------------------------------------------------------------------------------------------------
# latent-space tools (csrc/latent/latent.hip): pairs an eps apart, per-layer styles, the float64 pair distance
# --------------------------------------------------------------------------------------------------
def latent_pair(a, b, t, dt, mode, out0=None, out1=None):
    """The points of the path from row ``a[i]`` to row ``b[i]`` at ``t[i]`` and at ``t[i] + dt`` (the sum in float64), as two
    fp32 (n, d) tensors.  ``mode``: 0 lerp, 1 the slerp of Karras et al.  contrad_latent_pair's contract
    (include/contrad_hip.h)."""
    if not torch.is_tensor(a) or a.dim() != 2 or a.shape[0] < 1 or a.shape[1] < 1:
        raise RuntimeError('contrad_hip: latent_pair: a must be a non-empty (n, d) tensor')
    n, d = int(a.shape[0]), int(a.shape[1])
    _chk_dense(a, 'a', (n, d), torch.float32, a.device, 'latent_pair')
    _chk_dense(b, 'b', (n, d), torch.float32, a.device, 'latent_pair')
    _chk_dense(t, 't', (n,), torch.float32, a.device, 'latent_pair')
    if mode not in (0, 1):
        raise ValueError('latent_pair: mode 0 (lerp) or 1 (slerp) expected, got %r' % (mode,))
    if out0 is None:
        out0 = torch.empty((n, d), device=a.device, dtype=torch.float32)
    if out1 is None:
        out1 = torch.empty((n, d), device=a.device, dtype=torch.float32)
    _chk_dense(out0, 'out0', (n, d), torch.float32, a.device, 'latent_pair')
    _chk_dense(out1, 'out1', (n, d), torch.float32, a.device, 'latent_pair')
    lib().call('contrad_latent_pair', _p(a), _p(b), _p(t), float(dt), int(mode), _p(out0), _p(out1), ctypes.c_longlong(n), d,
               _stream())
    return out0, out1


def latent_styles(w, L, w2=None, cross=None, w_avg=None, psi=None, out=None):
    """Per-layer latents (B, L, d): ``w_avg + psi[l] * (src - w_avg)`` with ``src = w[b]`` for the layers ``l < cross[b]`` and
    ``w2[b]`` behind them.  ``cross``: (B,) fp32 on the device; ``w_avg``: (d,) or (1, d); ``psi``: (L,).  Without ``psi`` (and
    in every layer whose psi is 1) the rows are the source's bits.  contrad_latent_styles's contract."""
    if not torch.is_tensor(w) or w.dim() != 2 or w.shape[0] < 1 or w.shape[1] < 1 or int(L) < 1:
        raise RuntimeError('contrad_hip: latent_styles: w must be a non-empty (B, d) tensor and L at least 1')
    B, d, L = int(w.shape[0]), int(w.shape[1]), int(L)
    _chk_dense(w, 'w', (B, d), torch.float32, w.device, 'latent_styles')
    if (w2 is None) != (cross is None) or (w_avg is None) != (psi is None):
        raise RuntimeError('contrad_hip: latent_styles: w2 goes with cross, w_avg with psi')
    if w2 is not None:
        _chk_dense(w2, 'w2', (B, d), torch.float32, w.device, 'latent_styles')
        _chk_dense(cross, 'cross', (B,), torch.float32, w.device, 'latent_styles')
    if psi is not None:
        w_avg = w_avg.view(-1) if torch.is_tensor(w_avg) else w_avg
        _chk_dense(w_avg, 'w_avg', (d,), torch.float32, w.device, 'latent_styles')
        _chk_dense(psi, 'psi', (L,), torch.float32, w.device, 'latent_styles')
    if out is None:
        out = torch.empty((B, L, d), device=w.device, dtype=torch.float32)
    _chk_dense(out, 'out', (B, L, d), torch.float32, w.device, 'latent_styles')
    lib().call('contrad_latent_styles', _p(w), _p(w2), _p(w_avg), _p(psi), _p(cross), _p(out), B, L, d, _stream())
    return out


def pair_dist_resident_d():
    """The largest row length at which ``pair_dist`` keeps both rows in LDS (contrad_pair_dist_resident_d)."""
    return int(lib().raw('contrad_pair_dist_resident_d')())


def pair_dist(A, B, scale=1.0, out=None):
    """(n,) float64: ``scale * |A^_i - B^_i|^2`` of the normalised rows of two fp32 (n, d) matrices (row stride free, last
    stride 1), the difference taken first and everything in float64.  contrad_pair_dist's contract."""
    for name, m in (('A', A), ('B', B)):
        if not torch.is_tensor(m) or not m.is_cuda or m.dtype != torch.float32 or m.dim() != 2 or m.shape[0] < 1 or m.shape[1] < 1 \
                or m.stride(1) != 1 or m.stride(0) < m.shape[1]:
            raise RuntimeError('contrad_hip: pair_dist: %s must be a non-empty CUDA float32 (n, d) matrix with unit column stride' % name)
    if tuple(A.shape) != tuple(B.shape) or A.device != B.device:
        raise RuntimeError('contrad_hip: pair_dist: A %s and B %s must have one shape and device' % (tuple(A.shape), tuple(B.shape)))
    n, d = int(A.shape[0]), int(A.shape[1])
    if out is None:
        out = torch.empty((n,), device=A.device, dtype=torch.float64)
    _chk_dense(out, 'out', (n,), torch.float64, A.device, 'pair_dist')
    lib().call('contrad_pair_dist', _p(A), ctypes.c_longlong(A.stride(0)), _p(B), ctypes.c_longlong(B.stride(0)),
               ctypes.c_longlong(n), d, float(scale), _p(out), _stream())
    return out


# --------------------------------------------------------------------------------------------------
# StyleGAN2 projector (csrc/project/project.hip): the image end of the pixel-pyramid loss, the noise maps' gradient, the noise
# regulariser and the noise normalisation.  Scratch is a plain tensor sized by the formulas of include/contrad_hip.h.
# --------------------------------------------------------------------------------------------------
PROJ_MAX_LEVELS = 4


def proj_image_end_partial_floats(L, N, H, W):
    """Floats of ``proj_image_end``'s scratch: L * N * 3 * (H / rows), rows = 2^(L-1) doubled while 2 rows W <= 4096 and
    2 rows divides H (contrad_proj_image_end's contract)."""
    rows = 1 << (L - 1)
    while rows * 2 * W <= 4096 and H % (rows * 2) == 0:
        rows *= 2
    return L * N * 3 * (H // rows)


def proj_image_end(x, target, level_weights, pix=None, gx=None, partial=None):
    """(pix, gx): the rows ``pix[l][n] = mean(pool_l(x[n] - target[n]) ** 2)`` as an (L, N) tensor and
    ``gx = d sum_n sum_l level_weights[l] pix[l][n] / d x`` for NCHW fp32 ``x`` and ``target`` (N, 3, H, W); ``level_weights``:
    1 to 4 host floats.  contrad_proj_image_end's contract (include/contrad_hip.h)."""
    lam = [float(v) for v in level_weights]
    L = len(lam)
    if not 1 <= L <= PROJ_MAX_LEVELS:
        raise ValueError('proj_image_end: 1 to %d level weights expected, got %d' % (PROJ_MAX_LEVELS, L))
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3 or x.shape[0] < 1:
        raise RuntimeError('contrad_hip: proj_image_end: x must be a non-empty (N, 3, H, W) tensor')
    N, _, H, W = (int(v) for v in x.shape)
    _chk_dense(x, 'x', (N, 3, H, W), torch.float32, x.device, 'proj_image_end')
    _chk_dense(target, 'target', (N, 3, H, W), torch.float32, x.device, 'proj_image_end')
    T = 1 << (L - 1)
    if H % T or W % T:
        raise RuntimeError('contrad_hip: proj_image_end: %d levels need H and W divisible by %d, got %d x %d' % (L, T, H, W))
    if pix is None:
        pix = torch.empty((L, N), device=x.device, dtype=torch.float32)
    if gx is None:
        gx = torch.empty_like(x)
    nfl = proj_image_end_partial_floats(L, N, H, W)
    if partial is None:
        partial = torch.empty((nfl,), device=x.device, dtype=torch.float32)
    _chk_dense(pix, 'pix', (L, N), torch.float32, x.device, 'proj_image_end')
    _chk_dense(gx, 'gx', (N, 3, H, W), torch.float32, x.device, 'proj_image_end')
    _chk_dense(partial, 'partial', (nfl,), torch.float32, x.device, 'proj_image_end')
    lib().call('contrad_proj_image_end', _p(x), _p(target), (ctypes.c_float * L)(*lam), L, _p(pix), _p(gx), _p(partial),
               ctypes.c_longlong(nfl), N, H, W, _stream())
    return pix, gx


def proj_noise_grad(g_pre, noise_w, out=None):
    """(B, 1, H, W): ``noise_w * sum_k g_pre[b, h, w, k]`` of an NHWC gradient (B, H, W, K); ``noise_w``: the (1,) noise
    strength on the device.  contrad_proj_noise_grad's contract."""
    if not torch.is_tensor(g_pre) or g_pre.dim() != 4 or g_pre.numel() < 1:
        raise RuntimeError('contrad_hip: proj_noise_grad: g_pre must be a non-empty NHWC (B, H, W, K) tensor')
    B, H, W, K = (int(v) for v in g_pre.shape)
    _chk_dense(g_pre, 'g_pre', (B, H, W, K), torch.float32, g_pre.device, 'proj_noise_grad')
    _chk_dense(noise_w, 'noise_w', (1,), torch.float32, g_pre.device, 'proj_noise_grad')
    if out is None:
        out = torch.empty((B, 1, H, W), device=g_pre.device, dtype=torch.float32)
    _chk_dense(out, 'out', (B, 1, H, W), torch.float32, g_pre.device, 'proj_noise_grad')
    lib().call('contrad_proj_noise_grad', _p(g_pre), _p(noise_w), _p(out), ctypes.c_longlong(B * H * W), K, _stream())
    return out


def proj_noise_levels(R):
    """Levels of the noise regulariser on an R x R map: pooled while the side is above 8, the first level of side <= 8 counted."""
    J = 1
    while R > 8:
        R //= 2
        J += 1
    return J


def proj_noise_reg_scratch_floats(N, R):
    """Floats of ``proj_noise_reg``'s scratch: N * (sum_{j=1}^{J-1} (R / 2^j)^2 + 2 J ceil(R^2 / 4096) + 2 J)
    (contrad_proj_noise_reg's contract)."""
    J = proj_noise_levels(R)
    return N * (sum((R >> j) ** 2 for j in range(1, J)) + 2 * J * (-(-R * R // 4096)) + 2 * J)


def _chk_noise_map(m, who):
    if not torch.is_tensor(m) or m.dim() != 4 or m.shape[0] < 1 or m.shape[1] != 1 or m.shape[2] != m.shape[3]:
        raise RuntimeError('contrad_hip: %s: a non-empty (N, 1, R, R) map set expected' % who)
    N, R = int(m.shape[0]), int(m.shape[2])
    if R < 4 or R > 1024 or R & (R - 1):
        raise RuntimeError('contrad_hip: %s: R must be a power of two in [4, 1024], got %d' % (who, R))
    _chk_dense(m, 'map', (N, 1, R, R), torch.float32, m.device, who)
    return N, R


def proj_noise_reg(noise, g_acc, scale=1.0, reg=None, scratch=None):
    """reg (N,): the StyleGAN2 noise regulariser of every map of ``noise`` (N, 1, R, R); ``g_acc`` (same shape) receives
    ``+= scale * d reg[n] / d noise`` in place.  contrad_proj_noise_reg's contract."""
    N, R = _chk_noise_map(noise, 'proj_noise_reg')
    _chk_dense(g_acc, 'g_acc', (N, 1, R, R), torch.float32, noise.device, 'proj_noise_reg')
    if reg is None:
        reg = torch.empty((N,), device=noise.device, dtype=torch.float32)
    nfl = proj_noise_reg_scratch_floats(N, R)
    if scratch is None:
        scratch = torch.empty((nfl,), device=noise.device, dtype=torch.float32)
    _chk_dense(reg, 'reg', (N,), torch.float32, noise.device, 'proj_noise_reg')
    _chk_dense(scratch, 'scratch', (nfl,), torch.float32, noise.device, 'proj_noise_reg')
    lib().call('contrad_proj_noise_reg', _p(noise), _p(reg), _p(g_acc), float(scale), _p(scratch), ctypes.c_longlong(nfl), N, R,
               _stream())
    return reg


def proj_noise_normalize_(noise):
    """In place per map of ``noise`` (N, 1, R, R): subtract the mean, divide by the root of the mean square; a map of zero
    variance becomes zeros.  contrad_proj_noise_normalize's contract."""
    N, R = _chk_noise_map(noise, 'proj_noise_normalize_')
    lib().call('contrad_proj_noise_normalize', _p(noise), N, R, _stream())
    return noise
