"""Generates tests/golden/mc_stage_expected.npz with the REFERENCE's own marching-cubes extension
(oracle/_ref/marching_cubes_cpp.so, `make -C oracle ref`): its vertices, colours and faces on the stored stage cases of
tests/mc_cases.py (STAGE_CASES), among them the volumes in which every cube configuration occurs.  The volumes are
regenerated from their definitions by the tests, so only the reference's outputs are stored.
Authoring container only.

Usage:  make -C oracle ref && python tests/golden/make_golden_mc_stages.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'oracle', '_ref'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import marching_cubes_cpp as ref  # noqa: E402

from mc_cases import STAGE_CASES, make_stage_volume  # noqa: E402

OUT = os.path.join(HERE, 'mc_stage_expected.npz')


def main():
    out = {}
    for name, spec in STAGE_CASES.items():
        if not spec['stored']:
            continue
        tsdf, colors = make_stage_volume(spec)
        col = colors if colors is not None else torch.ones(tuple(tsdf.shape) + (3,), dtype=torch.uint8) * 220
        v, c, f = ref.run_marching_cubes(tsdf, col, spec['iso'], spec['trunc'], spec['thresh'])
        out[name + '_v'], out[name + '_c'], out[name + '_f'] = v.numpy(), c.numpy(), f.numpy()
        print(name, tuple(tsdf.shape), 'verts', len(v), 'faces', len(f))
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print('wrote %s: %d arrays, %d bytes' % (OUT, len(out), size))
    assert size < 1 << 20, 'the fixture has to stay under 1 MiB'


if __name__ == '__main__':
    main()
