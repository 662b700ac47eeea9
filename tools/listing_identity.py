"""Are two gfx950 device listings (hipcc --cuda-device-only -S) the same code in another order?  No GPU.

    python tools/listing_identity.py PARENT.s NEW.s

A host-side change that instantiates the kernels in another order moves whole functions in the listing and renumbers the
labels that carry the function's index (.LBB<n>_<m>, .Lfunc_end<n>); nothing else may differ.  The listing is cut into one
unit per symbol (body, its .amdhsa_kernel resource block, its .AMDGPU.csdata), the function index is taken out of the labels
and the name of the __hip_cuid_<hash> object is masked (it hashes the compilation, not the code).  Then: the same set of
symbols, every unit equal, the text before the first and after the last unit equal, and the metadata's kernel entries equal
as a set.  Prints one sha256 over the units sorted by symbol per file; exit status 0 exactly when all of that holds.
Behind profiles/wino_host_identity.txt.
"""
import hashlib
import re
import sys


def parts(path):
    lines = open(path).read().split('\n')
    lines = [re.sub(r'(\.L|\b)(BB|JTI)\d+_', r'\1\2_', re.sub(r'\.L(func_end|func_begin)\d+', r'.L\1', l)) for l in lines]
    lines = [re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_X', l) for l in lines]
    starts = [i for i, l in enumerate(lines)
              if l.startswith('\t.section\t.text.') and any('-- Begin function' in x for x in lines[i + 1:i + 4])]
    meta = next(i for i, l in enumerate(lines) if l.strip() == '.amdgpu_metadata')
    # the last unit ends with its .AMDGPU.csdata section: the `.set` lines behind it
    cs = next(i for i in range(starts[-1], meta) if lines[i].startswith('\t.section\t.AMDGPU.csdata'))
    end = next(i for i in range(cs + 1, meta) if lines[i].startswith('\t.') and not lines[i].startswith('\t.set'))
    units = {}
    for a, b in zip(starts, starts[1:] + [end]):
        units[lines[a].split('.text.')[1].split(',')[0]] = '\n'.join(lines[a:b])
    entries = re.split(r'\n(?=  - \.agpr_count)', '\n'.join(lines[meta:]))
    head, tail = entries[0], entries[-1].split('\namdhsa.target')[1]
    entries = sorted(e.split('\namdhsa.target')[0] for e in entries[1:])
    return units, '\n'.join(lines[:starts[0]]), '\n'.join(lines[end:meta]), head, entries, tail


def main(pa, pb):
    A, B = parts(pa), parts(pb)
    checks = [('symbols: %d / %d, the same set' % (len(A[0]), len(B[0])), set(A[0]) == set(B[0]))]
    differ = sorted(s for s in A[0] if s in B[0] and A[0][s] != B[0][s])
    checks.append(('units that differ: %d %s' % (len(differ), ' '.join(differ[:4])), not differ))
    kernels = [sum('.amdhsa_kernel' in u for u in X[0].values()) for X in (A, B)]
    checks.append(('.amdhsa_kernel blocks inside the units: %d / %d' % tuple(kernels), kernels[0] == kernels[1]))
    for name, i in (('text before the first unit', 1), ('text behind the last unit', 2), ('metadata head', 3),
                    ('metadata kernel entries (%d / %d, as a set)' % (len(A[4]), len(B[4])), 4), ('metadata tail', 5)):
        checks.append((name + ' equal', A[i] == B[i]))
    for text, ok in checks:
        print('%-9s %s' % ('ok' if ok else 'DIFFERENT', text))
    for X, p in ((A, pa), (B, pb)):
        print(hashlib.sha256('\n'.join(k + '\n' + X[0][k] for k in sorted(X[0])).encode()).hexdigest(), p)
    same = all(ok for _, ok in checks)
    print('identical per symbol' if same else 'NOT identical')
    return 0 if same else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
