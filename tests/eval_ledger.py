"""The ledger of csrc/eval/*.hip: the kernels of the evaluators that read no network (swd.hip), under the discipline of
tests/kernel_ledger.py -- every kernel instance the compiler emits is tied to the parity module that launches it, and
profiles/eval_ledger.txt records a dispatch count per instance from one kernel-trace-only profiler run of that module (no
counters in the same run).  Plain data and helpers, no GPU.  tests/kernel_ledger.py and profiles/kernel_ledger.txt pin
csrc/*.hip alone and are not touched by a new file under csrc/eval/.

The names below mirror kernel_ledger's, so tools/kernel_coverage.py --eval writes this record the way it writes the other:

    rocprofv3 --kernel-trace -f rocpd -d TRACE_DIR -o test_swd_kernels_gpu_%pid% -- python -m pytest tests/test_swd_kernels_gpu.py -q -m gpu
    python tools/kernel_coverage.py TRACE_DIR --eval
"""
import glob
import os

import kernel_ledger as KL

ROOT = KL.ROOT
CSRC = os.path.join(KL.CSRC, 'eval')
RECORD = os.path.join(ROOT, 'profiles', 'eval_ledger.txt')
NEVER = KL.NEVER
normalise = KL.normalise


def eval_objects():
    """The object files of csrc/eval/*.hip (build.py links them into both libraries)."""
    return [s[:-4] + '.o' for s in sorted(glob.glob(os.path.join(CSRC, '*.hip')))]


def instance_sources(objects=None):
    """{kernel instance: source name} of the eval object files (kernel_ledger.instance_sources on their list)."""
    return KL.instance_sources(eval_objects() if objects is None else objects)


def compiled_instances(objects=None):
    return set(instance_sources(objects))


PARITY_MODULES = {
    'test_swd_kernels_gpu': (('swd',), 'every kernel alone against tests/swd_ref64.py (float64 numpy and scipy) or exact host '
                                       'restatements (numpy indexing, np.sort, math.fsum), guard storage'),
}


def credited(module, source):
    return source in PARITY_MODULES[module][0]


# instance: the parity modules that launch it
LEDGER = {
    'swd_absdiff_kernel': ['test_swd_kernels_gpu'],
    'swd_final_kernel': ['test_swd_kernels_gpu'],
    'swd_gather_kernel': ['test_swd_kernels_gpu'],
    'swd_pyr_down_kernel': ['test_swd_kernels_gpu'],
    'swd_pyr_up_sub_kernel': ['test_swd_kernels_gpu'],
    'swd_sort_pass_kernel': ['test_swd_kernels_gpu'],
    'swd_sort_tile_kernel': ['test_swd_kernels_gpu'],
    'swd_u8_planes_kernel': ['test_swd_kernels_gpu'],
}

UNCOVERED = {}


def read_record(path=RECORD):
    """profiles/eval_ledger.txt as {instance: {module: count}} (kernel_ledger.read_record's format)."""
    return KL.read_record(path)
