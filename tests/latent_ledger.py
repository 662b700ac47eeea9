"""The ledger of csrc/latent/*.hip: the latent-space kernels (latent.hip), under the discipline of tests/kernel_ledger.py,
tests/eval_ledger.py and tests/spectral_ledger.py -- every kernel instance the compiler emits is tied to the parity module that
launches it, and profiles/latent_ledger.txt records a dispatch count per instance from one kernel-trace-only profiler run of
that module (no counters in the same run).  Plain data and helpers, no GPU.  The other three ledgers and their records pin
csrc/*.hip, csrc/eval/*.hip and csrc/spectral/*.hip alone and are not touched by a new file under csrc/latent/.

The names below mirror kernel_ledger's, so tools/kernel_coverage.py --latent writes this record the way it writes the others:

    rocprofv3 --kernel-trace -f rocpd -d TRACE_DIR -o test_latent_kernels_gpu_%pid% -- python -m pytest tests/test_latent_kernels_gpu.py -q -m gpu
    python tools/kernel_coverage.py TRACE_DIR --latent
"""
import glob
import os

import kernel_ledger as KL

ROOT = KL.ROOT
CSRC = os.path.join(KL.CSRC, 'latent')
RECORD = os.path.join(ROOT, 'profiles', 'latent_ledger.txt')
NEVER = KL.NEVER
normalise = KL.normalise


def latent_objects():
    """The object files of csrc/latent/*.hip (build.py links them into both libraries)."""
    return [s[:-4] + '.o' for s in sorted(glob.glob(os.path.join(CSRC, '*.hip')))]


def instance_sources(objects=None):
    """{kernel instance: source name} of the latent object files (kernel_ledger.instance_sources on their list)."""
    return KL.instance_sources(latent_objects() if objects is None else objects)


def compiled_instances(objects=None):
    return set(instance_sources(objects))


PARITY_MODULES = {
    'test_latent_kernels_gpu': (('latent',), 'every kernel alone against the float64 yardstick of tests/latent_ref64.py under its '
                                             'derived bounds: both modes of the pair kernel with its degenerate rows, the styles '
                                             'kernel with and without mixing and truncation, both paths of the pair distance, '
                                             'guard storage'),
}


def credited(module, source):
    return source in PARITY_MODULES[module][0]


# instance: the parity modules that launch it.  The template argument of pair_dist: the rows stay in LDS between the passes.
LEDGER = {
    'latent_pair_kernel': ['test_latent_kernels_gpu'],
    'latent_styles_kernel': ['test_latent_kernels_gpu'],
    'pair_dist_kernel<false>': ['test_latent_kernels_gpu'],
    'pair_dist_kernel<true>': ['test_latent_kernels_gpu'],
}

UNCOVERED = {}


def read_record(path=RECORD):
    """profiles/latent_ledger.txt as {instance: {module: count}} (kernel_ledger.read_record's format)."""
    return KL.read_record(path)
