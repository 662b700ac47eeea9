"""The ledger of csrc/project/*.hip: the loss ends of the StyleGAN2 projector (project.hip), under the discipline of
tests/kernel_ledger.py, tests/eval_ledger.py, tests/spectral_ledger.py and tests/latent_ledger.py -- every kernel instance the
compiler emits is tied to the parity module that launches it, and profiles/project_ledger.txt records a dispatch count per
instance from one kernel-trace-only profiler run of that module (no counters in the same run).  Plain data and helpers, no GPU.
The other four ledgers and their records pin csrc/*.hip, csrc/eval/*.hip, csrc/spectral/*.hip and csrc/latent/*.hip alone and
are not touched by a new file under csrc/project/.

The names below mirror kernel_ledger's, so tools/kernel_coverage.py --project writes this record the way it writes the others:

    rocprofv3 --kernel-trace -f rocpd -d TRACE_DIR -o test_project_kernels_gpu_%pid% -- python -m pytest tests/test_project_kernels_gpu.py -q -m gpu
    python tools/kernel_coverage.py TRACE_DIR --project
"""
import glob
import os

import kernel_ledger as KL

ROOT = KL.ROOT
CSRC = os.path.join(KL.CSRC, 'project')
RECORD = os.path.join(ROOT, 'profiles', 'project_ledger.txt')
NEVER = KL.NEVER
normalise = KL.normalise


def project_objects():
    """The object files of csrc/project/*.hip (build.py links them into both libraries)."""
    return [s[:-4] + '.o' for s in sorted(glob.glob(os.path.join(CSRC, '*.hip')))]


def instance_sources(objects=None):
    """{kernel instance: source name} of the project object files (kernel_ledger.instance_sources on their list)."""
    return KL.instance_sources(project_objects() if objects is None else objects)


def compiled_instances(objects=None):
    return set(instance_sources(objects))


PARITY_MODULES = {
    'test_project_kernels_gpu': (('project',), 'every kernel alone against the float64 yardstick of tests/project_ref64.py under its '
                                               'derived bounds: the image end at 1, 2 and 4 levels, both forms of the noise gradient, the '
                                               'regulariser on one and on several tiles, the normalisation with a constant map, guard '
                                               'storage around every output and the scratch'),
}


def credited(module, source):
    return source in PARITY_MODULES[module][0]


# instance: the parity modules that launch it.  The template argument of noise_grad: the rows are read as float4.
LEDGER = {
    'image_end_kernel': ['test_project_kernels_gpu'],
    'image_end_finish_kernel': ['test_project_kernels_gpu'],
    'noise_grad_kernel<false>': ['test_project_kernels_gpu'],
    'noise_grad_kernel<true>': ['test_project_kernels_gpu'],
    'reg_pyramid_kernel': ['test_project_kernels_gpu'],
    'reg_products_kernel': ['test_project_kernels_gpu'],
    'reg_finish_kernel': ['test_project_kernels_gpu'],
    'reg_grad_kernel': ['test_project_kernels_gpu'],
    'noise_normalize_kernel': ['test_project_kernels_gpu'],
}

UNCOVERED = {}


def read_record(path=RECORD):
    """profiles/project_ledger.txt as {instance: {module: count}} (kernel_ledger.read_record's format)."""
    return KL.read_record(path)
