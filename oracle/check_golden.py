#!/usr/bin/env python3
"""Generator <-> fixture consistency (build container only: needs the reference checkout).  Re-runs every golden generator
(`oracle/gen_golden*.py`) against the reference into a temporary directory and requires every committed fixture under tests/golden/
to be reproduced BIT FOR BIT, key for key.  Catches a generator edited without re-committing its fixtures (and vice versa).

    VKN_REFERENCE=<reference checkout> python oracle/check_golden.py        # exit status 0: in sync
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
GENERATORS = ('gen_golden.py', 'gen_golden_vis.py', 'gen_golden_tracker.py', 'gen_golden_api.py')


def _same(a, b):
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind in 'fc':
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(a, b)


def compare(fresh_dir):
    """The differences between the committed fixtures and those in `fresh_dir`, one line each."""
    committed = sorted(f for f in os.listdir(GOLDEN) if f.endswith(('.npz', '.json')))
    fresh = sorted(f for f in os.listdir(fresh_dir) if f.endswith(('.npz', '.json')))
    bad = []
    if committed != fresh:
        bad.append(f'fixtures without a generator: {sorted(set(committed) - set(fresh))}; '
                   f'generated but not committed: {sorted(set(fresh) - set(committed))}')
    for f in sorted(set(committed) & set(fresh)):
        if f.endswith('.json'):
            with open(os.path.join(GOLDEN, f)) as fa, open(os.path.join(fresh_dir, f)) as fb:
                if json.load(fa) != json.load(fb):
                    bad.append(f)
            continue
        a, b = np.load(os.path.join(GOLDEN, f)), np.load(os.path.join(fresh_dir, f))
        if sorted(a.files) != sorted(b.files):
            bad.append(f'{f}: keys differ (committed - fresh = {sorted(set(a.files) - set(b.files))}, '
                       f'fresh - committed = {sorted(set(b.files) - set(a.files))})')
            continue
        bad += [f'{f}[{k}]' for k in a.files if not _same(a[k], b[k])]
    return bad


def main():
    ref = os.environ.get('VKN_REFERENCE')
    if not ref or not os.path.isdir(os.path.join(ref, 'knet')):
        raise SystemExit('set VKN_REFERENCE to the reference checkout')
    with tempfile.TemporaryDirectory(prefix='golden_regen_') as out:
        env = dict(os.environ, VKN_GOLDEN_OUT=out, VKN_REFERENCE=ref, PYTHONDONTWRITEBYTECODE='1')
        for g in GENERATORS:
            r = subprocess.run([sys.executable, os.path.join(HERE, g)], env=env, capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise SystemExit(f'{g} failed:\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}')
        bad = compare(out)
    if bad:
        raise SystemExit('generator and fixtures are out of sync:\n  ' + '\n  '.join(bad))
    print('every fixture under tests/golden/ is reproduced bit for bit')


if __name__ == '__main__':
    main()
