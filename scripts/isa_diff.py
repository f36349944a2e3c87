#!/usr/bin/env python3
"""Same machine code?  Device assembly of every file of build.SOURCES, a git revision against the working tree.

    python scripts/isa_diff.py [REV]          (REV defaults to HEAD~1; needs hipcc and git, no GPU)

REV's env_build_amd/csrc and include are written to a temporary directory with `git archive`; every file of build.SOURCES is compiled
in both trees with hipcc + build.FLAGS + --cuda-device-only -S and the two texts are compared.  Lines naming the __hip_cuid_ symbol
(a per-compilation id) are left out; everything else counts: instructions, .amdhsa_ blocks, register, LDS and scratch figures,
metadata.  differ = lines of either text that the other does not have (as a multiset; the same lines in another order also count).
Prints the table of profiles/r13_tape_refactor_isa.txt with a hash of each text, and build.kernel_hash of both trees; exit status 1 if
anything differs.  The file list and the flags are this tree's: a file REV does not have differs in every line."""
import collections
import hashlib
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from env_build_amd import build  # noqa: E402

HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')


def assembly(job):
    src, out = job
    if not os.path.isfile(src):
        return []
    subprocess.run([HIPCC] + build.FLAGS + ['--cuda-device-only', '-S', src, '-o', out], check=True)
    with open(out) as fh:
        return [ln for ln in fh if '__hip_cuid' not in ln]


def main():
    rev = sys.argv[1] if len(sys.argv) > 1 else 'HEAD~1'
    with tempfile.TemporaryDirectory(prefix='isa_diff_') as tmp:
        archive = subprocess.Popen(['git', '-C', ROOT, 'archive', rev, 'env_build_amd/csrc', 'include'], stdout=subprocess.PIPE)
        subprocess.run(['tar', '-x', '-C', tmp], stdin=archive.stdout, check=True)
        trees = {'rev': os.path.join(tmp, 'env_build_amd', 'csrc'), 'tree': build.CSRC}
        jobs = [(os.path.join(trees[t], f), os.path.join(tmp, '%s_%s.s' % (t, f))) for f in build.SOURCES for t in ('rev', 'tree')]
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            texts = list(pool.map(assembly, jobs))
        hashes = {}
        for t, csrc in trees.items():
            build.CSRC = csrc
            hashes[t] = {k: build.kernel_hash(k) for k in build.KERNEL_SOURCES}
    bad = 0
    print('# %s against the working tree; hipcc %s --cuda-device-only -S' % (rev, ' '.join(build.FLAGS)))
    print('# ' + subprocess.check_output([HIPCC, '--version'], text=True).splitlines()[0])
    print('%-34s %8s %8s %8s  %s' % ('file', 'kernels', 'lines', 'differ', 'sha256'))
    for n, f in enumerate(build.SOURCES):
        old, new = texts[2 * n], texts[2 * n + 1]
        a, b = collections.Counter(old), collections.Counter(new)
        differ = 0 if old == new else max(sum((a - b).values()) + sum((b - a).values()), 1)
        bad += differ
        print('%-34s %8d %8d %8d  %s' % (f, sum(ln.lstrip().startswith('.amdhsa_kernel ') for ln in new), len(new), differ,
                                         hashlib.sha256(''.join(new).encode()).hexdigest()[:16]))
    print()
    for k in build.KERNEL_SOURCES:
        same = hashes['rev'][k] == hashes['tree'][k]
        bad += not same
        print('build.kernel_hash(%s) = %s  (%s: %s)' % (k, hashes['tree'][k], rev, 'equal' if same else hashes['rev'][k]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
