"""Dev tool: where the time of a power-spectrum evaluation (contrad_amd/spectrum.py, csrc/spectral/spectrum.hip) goes.

    python tools/bench_spectrum.py kernels [OUT.txt]   # every kernel at the CIFAR shape (n = 16384, 32 x 32) and at n = 2048 of 512 x 512
    python tools/bench_spectrum.py whole   [OUT.txt]   # spectrum_of wall time and peak memory at both shapes

Times are HIP-event medians over repeated windows with the min - max spread, one process, one configuration at a time.
Every kernel is held against its bytes model at 6.3 TB/s (the achievable HBM rate): rfft2 reads 3 n S^2 bytes and writes
8 n S (S / 2 + 1) (the two-pass sizes read and write the spectrum once more), radial and mean_map read the spectrum once.
For comparison only, ``torch.fft.rfft2`` on the same luma planes (fp32, already converted: it does less) is timed in the same
process, alternating with ours, where the installed torch provides it on this device.
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_knn import fmt, windows  # noqa: E402
from contrad_amd import ops, spectrum  # noqa: E402

dev = torch.device('cuda', 0)
HBM = 6.3e12
SHAPES = ((16384, 32), (2048, 512))


def model(nbytes, t):
    """'... GB/s, x.xx of the bytes model' for a median of t[0] milliseconds."""
    return '  %6.0f GB/s = %.2f of the %.0f MB model at 6.3 TB/s' % (nbytes / t[0] * 1e-6, nbytes / HBM / (t[0] * 1e-3), nbytes * 1e-6)


def kernels(emit):
    for n, S in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        m = n                                                              # (the whole set in one call: 2.2 GB of spec at 512 x 512)
        x = torch.randint(0, 256, (m, S, S, 3), generator=g, dtype=torch.uint8, device=dev)
        tw, bins, rcount = spectrum.device_tables(S, dev)
        spec = ops.spec_rfft2(x, tw)
        spec_bytes = spec.numel() * 4
        passes = 3 if S > 128 else 1
        iters = 5 if S > 128 else 20
        emit('--- n = %d of %d x %d in one call: spec is %.0f MB' % (n, S, S, spec_bytes * 1e-6))
        t = windows(lambda: ops.spec_rfft2(x, tw, out=spec), iters=iters)
        emit(fmt('spec_rfft2 %d x %d x %d (%s)' % (m, S, S, 'rows + columns in place' if S > 128 else 'fused in LDS'), t,
                 model(x.numel() + passes * spec_bytes, t)))
        luma = (x.float() * torch.tensor([77.0, 150.0, 29.0], device=dev)).sum(dim=3) / 256.0
        try:
            ref = torch.fft.rfft2(luma)
            err = float((torch.view_as_real(ref) - spec).abs().max())
            for rnd in range(2):                                           # alternating
                t = windows(lambda: torch.fft.rfft2(luma), iters=iters, reps=5)
                emit(fmt('  torch.fft.rfft2 on the fp32 luma planes, round %d (max |difference| to ours %.3g)' % (rnd, err), t,
                         model(luma.numel() * 4 + spec_bytes, t)))
                t = windows(lambda: ops.spec_rfft2(x, tw, out=spec), iters=iters, reps=5)
                emit(fmt('  spec_rfft2, round %d' % rnd, t))
            del ref
        except Exception as e:                                             # (the installed torch may not ship an FFT for this device)
            emit('  torch.fft.rfft2 is not available on this device: %s' % (str(e).splitlines() or [type(e).__name__])[0])
        del luma
        ops.spec_rfft2(x, tw, out=spec)
        prof = ops.spec_radial(spec, bins, rcount)
        t = windows(lambda: ops.spec_radial(spec, bins, rcount, out=prof), iters=iters)
        emit(fmt('spec_radial -> [%d][%d]' % (m, prof.shape[1]), t, model(spec_bytes, t)))
        mp = ops.spec_mean_map(spec)
        t = windows(lambda: ops.spec_mean_map(spec, out=mp), iters=iters)
        emit(fmt('spec_mean_map -> [%d][%d]' % (S, S // 2 + 1), t, model(spec_bytes, t)))
        del spec, x, prof, mp
        torch.cuda.empty_cache()


def whole(emit):
    for n, S in SHAPES:
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randint(0, 256, (n, S, S, 3), generator=g, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        times = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.time()
            out = spectrum.spectrum_of(x)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        emit('spectrum_of n = %d, %d x %d, chunks of %d: %.3f s (min %.3f, max %.3f) wall, first call included; peak device memory '
             '%.2f GB beside the %.2f GB of images; mean[1] %.4f'
             % (n, S, S, min(n, spectrum.default_chunk(S)), float(np.median(times)), min(times), max(times),
                (torch.cuda.max_memory_allocated() - base) * 1e-9, base * 1e-9, out['mean'][1]))
        del x, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    mode = sys.argv[1] if len(sys.argv) > 1 else 'kernels'
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)
    {'kernels': kernels, 'whole': whole}[mode](emit)
    if len(sys.argv) > 2:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[2])) or '.', exist_ok=True)
        with open(sys.argv[2], 'a') as f:
            f.write('\n'.join(lines) + '\n')
