"""bench.py's options around the headline (CPU): `--full` and `--dump-outputs` exist, and the dump writes float32 arrays within its byte
budget — small outputs whole, large ones as the same seeded sample on every run."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_outputs_options_exist():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert '--full' in r.stdout and '--dump-outputs' in r.stdout


def test_dump_outputs_whole_small_arrays_and_seeded_samples_of_large_ones(tmp_path):
    import bench
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    big = torch.randn(bench.DUMP_BYTES // 4 + 1000, generator=torch.Generator().manual_seed(0))
    arrays = {'small': small, 'big': big, 'ints': torch.arange(5)}
    bench.dump_outputs(str(tmp_path / 'a'), arrays)
    bench.dump_outputs(str(tmp_path / 'b'), arrays)
    total = 0
    for name in arrays:
        a, b = np.load(tmp_path / 'a' / f'{name}.npy'), np.load(tmp_path / 'b' / f'{name}.npy')
        assert a.dtype == np.float32 and np.array_equal(a, b), name
        total += os.path.getsize(tmp_path / 'a' / f'{name}.npy')
    assert total <= 64 << 20
    assert np.array_equal(np.load(tmp_path / 'a' / 'small.npy'), small.float().numpy())
    assert np.array_equal(np.load(tmp_path / 'a' / 'ints.npy'), np.arange(5, dtype=np.float32))
    s = np.load(tmp_path / 'a' / 'big.npy')
    assert s.ndim == 1 and s.size == bench.DUMP_BYTES // 4 // len(arrays)
    assert np.isin(s, big.numpy()).all()            # a sample of the tensor's own elements
