"""Dev tool: writes tests/golden/fd.npz, the fixture of tests/test_fd_ref64_cpu.py -- small float64 feature matrices and the
value the reference's ``calculate_frechet_distance(mean, np.cov(rows, rowvar=False), ...)`` returns for them.

    python tools/make_fd_golden.py REFERENCE_ROOT [OUT.npz]

The reference's third_party/fid/fid_score.py imports its Inception network (torchvision) at the top of the file; only the
distance function is wanted, so a stub module of this tool's own stands in for that import.  Needs scipy (the reference
takes ``scipy.linalg.sqrtm``).  The fixture holds data only: ``real_<i>``, ``fake_<i>`` and ``fd`` [n_cases]."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(40, 33, 12), (64, 50, 16), (25, 31, 6), (200, 150, 24)]        # (n_r, n_f, d): full rank, n > d


def reference_distance(reference_root):
    stub = types.ModuleType('inception')
    stub.InceptionV3 = None                                               # never called: only the distance function is used
    for name in ('third_party.fid.inception', 'inception'):
        sys.modules[name] = stub
    for name in ('third_party', 'third_party.fid'):
        sys.modules.setdefault(name, types.ModuleType(name))
    spec = importlib.util.spec_from_file_location('reference_fid_score', os.path.join(reference_root, 'third_party', 'fid', 'fid_score.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.calculate_frechet_distance


def sets(i, n_r, n_f, d):
    r = np.random.RandomState(100 + i)
    real = np.maximum(r.randn(n_r, d) @ r.randn(d, d) * 0.3 + 0.2, 0.0)
    fake = np.maximum(r.randn(n_f, d) @ r.randn(d, d) * 0.3 + 0.4, 0.0)
    norm = lambda x: x / np.sqrt((x * x).sum(1, keepdims=True))
    return norm(real + 1e-3), norm(fake + 1e-3)


def main(argv):
    distance = reference_distance(argv[1])
    out = argv[2] if len(argv) > 2 else os.path.join(ROOT, 'tests', 'golden', 'fd.npz')
    arrays, values = {}, []
    for i, (n_r, n_f, d) in enumerate(CASES):
        real, fake = sets(i, n_r, n_f, d)
        arrays['real_%d' % i], arrays['fake_%d' % i] = real, fake
        values.append(float(distance(real.mean(0), np.cov(real, rowvar=False), fake.mean(0), np.cov(fake, rowvar=False))))
        print('case %d (%d real, %d fake, d = %d): %.15g' % (i, n_r, n_f, d, values[-1]))
    np.savez(out, fd=np.asarray(values, np.float64), **arrays)
    print('wrote %s (%d bytes)' % (out, os.path.getsize(out)))


if __name__ == '__main__':
    main(sys.argv)
