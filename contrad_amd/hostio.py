"""Host -> device hand-over of the per-step random draws (latents, augmentation parameters).

The draws happen on the host in the reference's RNG order; what this module controls is only HOW the few hundred KB
reach the GPU.  A synchronous pageable ``tensor.to(device)`` makes the host wait until the GPU has drained everything
queued before it -- twice per step the GPU then idles until the next kernels are enqueued (0.6 ms of a 4.1 ms step at
a per-rank batch of 64, 0.5 of 18.1 ms at 512).  ``upload()`` instead copies into a small ring of pinned staging
buffers and lets a kernel pull the data over PCIe from the device-mapped pinned memory (stream-ordered, no runtime
copy), and ``StepThrottle`` keeps the host at most ONE step ahead of the GPU.

Two ROCm 7.2 observations are built in (tools/host_time.py, bench.py --dev-local-batch):
  * a single asynchronous hand-over of more than ~128 KB -- hipMemcpyAsync from pinned memory or the pull kernel alike --
    makes every following step take 2-3x as long (33-53 instead of 18 ms at batch 512, where the latent block is
    256 KB); pieces of 64 KB do not.  Cause not understood; big tensors therefore go in 64 KB pieces.
  * unbounded host run-ahead (>= 3 steps queued) makes the runtime drain its queue every third step; hence the throttle.

Measured step times, synchronous -> asynchronous (1 GPU, SNDCGAN D-step, per-rank batch 1024 / 512 / 256 / 128 / 64):
37.5 -> 33.9, 18.1 -> 17.6, 10.0 -> 9.5, 6.1 -> 5.5, 4.1 -> 3.5 ms.   CONTRAD_SYNC_UPLOADS=1 restores the synchronous path.
"""
import os

import torch

_SYNC = os.environ.get('CONTRAD_SYNC_UPLOADS', '0') == '1'
_CHUNK = int(os.environ.get('CONTRAD_UPLOAD_CHUNK', str(64 * 1024)))     # bytes per asynchronous piece
_RING = 8                      # staging slots per (shape, dtype); a slot is only reused after its own pull has completed
_rings = {}


def _pull(t, device, out=None):
    """One piece: host tensor -> pinned ring slot -> device tensor (``out``: a contiguous device tensor of t's shape, else
    a new one) written by contrad_pull_host on the current stream."""
    from . import ops
    key = (tuple(t.shape), t.dtype)
    ring = _rings.get(key)
    if ring is None:
        ring = _rings[key] = [[[torch.empty(t.shape, dtype=t.dtype).pin_memory(), None] for _ in range(_RING)], 0]
    slots, i = ring
    ring[1] = (i + 1) % _RING
    buf, done = slots[i]
    if done is not None:
        done.synchronize()     # (returns at once unless the caller is more than _RING uploads ahead of the GPU)
    buf.copy_(t)
    if out is None:
        out = torch.empty(t.shape, dtype=t.dtype, device=device)
    ops.lib().call('contrad_pull_host', buf.data_ptr(), out.data_ptr(), t.numel(), ops._stream())
    slots[i][1] = torch.cuda.Event()
    slots[i][1].record()
    return out


def upload(t, device):
    """CPU float32 tensor -> device tensor, stream-ordered on the current stream, without a host-side wait."""
    if _SYNC or t.dtype != torch.float32 or torch.device(device).type != 'cuda':
        return t.to(device)
    nbytes = t.numel() * t.element_size()
    if nbytes <= _CHUNK or t.dim() != 2:
        return _pull(t.contiguous(), device) if nbytes <= 2 * _CHUNK else t.to(device)
    rows = max(1, _CHUNK // (t.shape[1] * t.element_size()))
    return torch.cat([_pull(t[i:i + rows].contiguous(), device) for i in range(0, t.shape[0], rows)], 0)


def upload_into(t, dst):
    """``dst.copy_(upload(t, dst.device))`` without the temporaries: the pieces are pulled straight into (row slices of)
    the contiguous device tensor ``dst`` -- a captured step's static inputs -- instead of into new tensors that are then
    concatenated and copied.  Same piece sizes as upload()."""
    if (_SYNC or t.dtype != torch.float32 or dst.dtype != torch.float32 or dst.device.type != 'cuda'
            or not dst.is_contiguous() or tuple(dst.shape) != tuple(t.shape)):
        dst.copy_(upload(t, dst.device).view(dst.shape))
        return
    nbytes = t.numel() * t.element_size()
    if nbytes <= _CHUNK or t.dim() != 2:
        if nbytes <= 2 * _CHUNK:
            _pull(t.contiguous(), dst.device, out=dst)
        else:
            dst.copy_(t)
        return
    rows = max(1, _CHUNK // (t.shape[1] * t.element_size()))
    for i in range(0, t.shape[0], rows):
        _pull(t[i:i + rows].contiguous(), dst.device, out=dst[i:i + rows])


class StepThrottle(object):
    """Bounds the host's run-ahead to one step: ``begin()`` at the top of a step waits for the end of the step before the
    previous one, ``end()`` marks the end of this step's launches."""

    def __init__(self):
        self.events = []
        self.depth = 0                      # re-entrant: a step function called inside a throttled iteration is a no-op

    def begin(self):
        self.depth += 1
        if self.depth > 4:                  # no step nests this deep: an exception left the counter stuck -- start over
            self.depth = 1
        if self.depth > 1:
            return
        while len(self.events) >= 2:
            self.events.pop(0).synchronize()

    def end(self):
        self.depth = max(self.depth - 1, 0)
        if _SYNC or self.depth > 0:
            return
        e = torch.cuda.Event()
        e.record()
        self.events.append(e)


THROTTLE = StepThrottle()


# ---- image files (sample writers; no torchvision / PIL here) ----
def to_uint8(x):
    """Quantise [0, 1] floats as torchvision's ``save_image`` does: x * 255 + 0.5, clamped to [0, 255], truncated."""
    return x.mul(255.0).add_(0.5).clamp_(0, 255).to(torch.uint8)


def _png_chunk(tag, data):
    import struct
    import zlib
    return struct.pack('>I', len(data)) + tag + data + struct.pack('>I', zlib.crc32(tag + data) & 0xffffffff)


def _png_rows(img, who):
    """(height, width, the filter-type-0 scanlines) of a uint8 (H, W, 3) array."""
    import numpy as np
    img = np.ascontiguousarray(img)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
        raise ValueError('%s: uint8 (H, W, 3) expected, got %s %s' % (who, img.dtype, img.shape))
    h, w, _ = img.shape
    return h, w, np.concatenate([np.zeros((h, 1), np.uint8), img.reshape(h, w * 3)], axis=1).tobytes()


def png_bytes(img):
    """An 8-bit RGB PNG (one IDAT chunk, filter type 0 on every row) of a uint8 (H, W, 3) array."""
    import struct
    import zlib
    h, w, raw = _png_rows(img, 'png_bytes')
    return (b'\x89PNG\r\n\x1a\n' + _png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0))
            + _png_chunk(b'IDAT', zlib.compress(raw, 6)) + _png_chunk(b'IEND', b''))


def apng_bytes(frames, delay_ms=500, deflated=None):
    """An animated PNG (APNG 1.0: ``acTL``, then ``fcTL`` + ``IDAT`` for the first frame and ``fcTL`` + ``fdAT`` for every
    later one, one sequence-number series over the fcTL / fdAT chunks) of uint8 (H, W, 3) arrays of one size, each shown for
    ``delay_ms``, looping forever.  The first frame is the still image a plain PNG reader shows.  ``deflated``: a list the
    caller keeps between calls with a growing ``frames`` -- it holds the compressed scanlines of the frames seen so far,
    so that rewriting a training run's animation deflates only the new frames."""
    import struct
    import zlib
    frames = list(frames)
    if not frames:
        raise ValueError('apng_bytes: at least one frame')
    if not 0 < int(delay_ms) < 65536:
        raise ValueError('apng_bytes: delay_ms in [1, 65535], got %r' % (delay_ms,))
    cache = deflated if deflated is not None else []
    size = None
    for i, f in enumerate(frames):
        if i < len(cache):
            h, w = f.shape[0], f.shape[1]
        else:
            h, w, raw = _png_rows(f, 'apng_bytes')
            cache.append(zlib.compress(raw, 6))
        if size is None:
            size = (h, w)
        elif size != (h, w):
            raise ValueError('apng_bytes: frame %d is %s, frame 0 is %s' % (i, (h, w), size))
    h, w = size
    out = [b'\x89PNG\r\n\x1a\n', _png_chunk(b'IHDR', struct.pack('>IIBBBBB', w, h, 8, 2, 0, 0, 0)),
           _png_chunk(b'acTL', struct.pack('>II', len(frames), 0))]
    seq = 0
    for i in range(len(frames)):
        # full-canvas frame at (0, 0), delay_ms / 1000 s, dispose: none, blend: source
        out.append(_png_chunk(b'fcTL', struct.pack('>IIIIIHHBB', seq, w, h, 0, 0, int(delay_ms), 1000, 0, 0)))
        seq += 1
        if i == 0:
            out.append(_png_chunk(b'IDAT', cache[0]))
        else:
            out.append(_png_chunk(b'fdAT', struct.pack('>I', seq) + cache[i]))
            seq += 1
    out.append(_png_chunk(b'IEND', b''))
    return b''.join(out)


def write_png(path, img):
    with open(path, 'wb') as f:
        f.write(png_bytes(img))
