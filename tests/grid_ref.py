"""Yardstick of csrc/imagegrid.hip: torchvision's ``make_grid(images, nrow, padding, pad_value=pad_value)`` followed by
``save_image``'s quantisation, restated from their documented semantics in numpy, the quantisation through torch CPU ops
(``mul(255).add_(0.5).clamp_(0, 255).to(uint8)``).  One deviation, shared with the kernel: a single image is framed like
any other batch (torchvision returns it as it is)."""
import numpy as np
import torch


def quantise(x):
    """save_image's bytes of a float array (any shape)."""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    return t.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy()


def grid_ref(images, nrow=8, padding=2, pad_value=0.0):
    """uint8 (rows, columns, 3) canvas of float (n, 3, H, W) ``images`` (numpy array or CPU tensor)."""
    x = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    x = x.astype(np.float32, copy=False)
    n, c, H, W = x.shape
    assert c == 3 and n > 0
    xmaps = min(nrow, n)
    ymaps = -(-n // xmaps)
    ch, cw = H + padding, W + padding
    canvas = np.full((3, ymaps * ch + padding, xmaps * cw + padding), pad_value, np.float32)
    for k in range(n):
        y0, x0 = padding + (k // xmaps) * ch, padding + (k % xmaps) * cw
        canvas[:, y0:y0 + H, x0:x0 + W] = x[k]
    return quantise(canvas.transpose(1, 2, 0))


def batch_ref(images):
    """uint8 (n, H, W, 3) of float (n, 3, H, W) images."""
    x = images.detach().cpu().numpy() if torch.is_tensor(images) else np.asarray(images)
    return quantise(x.astype(np.float32, copy=False).transpose(0, 2, 3, 1))
