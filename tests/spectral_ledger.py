"""The ledger of csrc/spectral/*.hip: the frequency-domain kernels (spectrum.hip), under the discipline of
tests/kernel_ledger.py and tests/eval_ledger.py -- every kernel instance the compiler emits is tied to the parity module that
launches it, and profiles/spectral_ledger.txt records a dispatch count per instance from one kernel-trace-only profiler run of
that module (no counters in the same run).  Plain data and helpers, no GPU.  The other two ledgers and their records pin
csrc/*.hip and csrc/eval/*.hip alone and are not touched by a new file under csrc/spectral/.

The names below mirror kernel_ledger's, so tools/kernel_coverage.py --spectral writes this record the way it writes the others:

    rocprofv3 --kernel-trace -f rocpd -d TRACE_DIR -o test_spectrum_kernels_gpu_%pid% -- python -m pytest tests/test_spectrum_kernels_gpu.py -q -m gpu
    python tools/kernel_coverage.py TRACE_DIR --spectral
"""
import glob
import os

import kernel_ledger as KL

ROOT = KL.ROOT
CSRC = os.path.join(KL.CSRC, 'spectral')
RECORD = os.path.join(ROOT, 'profiles', 'spectral_ledger.txt')
NEVER = KL.NEVER
normalise = KL.normalise


def spectral_objects():
    """The object files of csrc/spectral/*.hip (build.py links them into both libraries)."""
    return [s[:-4] + '.o' for s in sorted(glob.glob(os.path.join(CSRC, '*.hip')))]


def instance_sources(objects=None):
    """{kernel instance: source name} of the spectral object files (kernel_ledger.instance_sources on their list)."""
    return KL.instance_sources(spectral_objects() if objects is None else objects)


def compiled_instances(objects=None):
    return set(instance_sources(objects))


PARITY_MODULES = {
    'test_spectrum_kernels_gpu': (('spectrum',), 'every kernel alone: the transform against numpy.fft.rfft2 of the exact luma in '
                                                 'float64 under the derived bound of tests/spectrum_ref64.py, the two reductions '
                                                 'against float64 numpy on the device\'s own spectrum, guard storage'),
}


def credited(module, source):
    return source in PARITY_MODULES[module][0]


# instance: the parity modules that launch it.  The template arguments: log2 S, images per workgroup (fused kernel), threads.
LEDGER = {
    'spec_mean_map_kernel': ['test_spectrum_kernels_gpu'],
    'spec_radial_kernel': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_cols_kernel<8, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_cols_kernel<9, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_fused_kernel<4, 16, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_fused_kernel<5, 4, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_fused_kernel<6, 1, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_fused_kernel<7, 1, 512>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_rows_kernel<8, 256>': ['test_spectrum_kernels_gpu'],
    'spec_rfft2_rows_kernel<9, 256>': ['test_spectrum_kernels_gpu'],
}

UNCOVERED = {}


def read_record(path=RECORD):
    """profiles/spectral_ledger.txt as {instance: {module: count}} (kernel_ledger.read_record's format)."""
    return KL.read_record(path)
