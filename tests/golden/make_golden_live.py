"""Generates tests/golden/live_reference.npz: what the REAL reference code returns on the seeded random inputs of
tests/live_cases.py — /root/reference/torch/data_util.py (load_train_file, load_scene, load_scene_known) and loss.py
(compute_iou_sparse_dense, compute_l1_tgtsurf_sparse_dense), unmodified, and the reference's marching-cubes extension
(oracle/_ref/marching_cubes_cpp.so, `make -C oracle ref`).  Authoring container only; the fixture travels, the reference
does not.  Outputs too large to store whole (the two scene-size meshes) are stored as shapes + sha256 digests.

Substituted at import time: `sparseconvnet`, `plyfile`, `marching_cubes` (+ `.marching_cubes`) := empty stubs
(visualisation only, as in make_golden_data.py).

Usage:  python tests/golden/make_golden_live.py
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS, os.path.join(ROOT, 'oracle', '_ref')):
    sys.path.insert(0, p)

for name in ('sparseconvnet', 'plyfile'):
    sys.modules[name] = types.ModuleType(name)
pkg = types.ModuleType('marching_cubes')
pkg.marching_cubes = types.ModuleType('marching_cubes.marching_cubes')
sys.modules['marching_cubes'] = pkg
sys.modules['marching_cubes.marching_cubes'] = pkg.marching_cubes
sys.path.insert(0, '/root/reference/torch')
import data_util as ref_data        # noqa: E402
import loss as ref_loss             # noqa: E402
import marching_cubes_cpp as ref_mc  # noqa: E402

import live_cases as L              # noqa: E402


def main():
    out = {}
    for seed in range(4):                                        # test_oracle_data
        with tempfile.TemporaryDirectory() as tmp:
            chunk, s_tgt, knw = L.data_files(tmp, seed)
            out['data%d_chunk_sha' % seed] = np.array(L.file_digest(chunk))
            out['data%d_scene_sha' % seed] = np.array(L.file_digest(s_tgt))
            for k, v in L.train_fields(ref_data.load_train_file(chunk)).items():
                out['data%d_train_%s' % (seed, k)] = v
            for k, v in L.scene_fields(ref_data.load_scene(s_tgt), ref_data.load_scene_known(knw)).items():
                out['data%d_scene_%s' % (seed, k)] = v
    for seed in range(4):                                        # test_oracle_metrics
        occ, pred, sdf, known, locs, vals = L.metrics_inputs(seed)
        tgt_b, tpred = torch.from_numpy(occ.astype(np.uint8)), [torch.from_numpy(p) for p in pred]
        for masking in (True, False):
            out['metrics%d_iou_m%d' % (seed, masking)] = np.array(ref_loss.compute_iou_sparse_dense(tpred, tgt_b, masking))
            out['metrics%d_iou_per_m%d' % (seed, masking)] = np.asarray(
                ref_loss.compute_iou_sparse_dense(tpred, tgt_b, masking, batched=False))
        out['metrics%d_l1' % seed] = np.array([
            ref_loss.compute_l1_tgtsurf_sparse_dense(torch.from_numpy(locs), torch.from_numpy(vals), torch.from_numpy(sdf),
                                                     3.0, masking, torch.from_numpy(known), thresh=thresh)
            for masking, thresh in L.L1_CASES], dtype=np.float64)
    for seed in range(6):                                        # test_oracle_mc
        vol, colors, iso, trunc, thresh = L.mc_volume(seed)
        v, c, f = ref_mc.run_marching_cubes(torch.from_numpy(vol), torch.from_numpy(colors), iso, trunc, thresh)
        out['mc%d_v' % seed], out['mc%d_c' % seed], out['mc%d_f' % seed] = v.numpy(), c.numpy(), f.numpy()
    vols, col = L.mc_scene_volumes()                             # test_gpu_marching_cubes, scene size
    for i, tsdf in enumerate(vols):
        v, c, f = (t.numpy() for t in ref_mc.run_marching_cubes(tsdf, col, 0.0, 3.0, 10.0))
        out['mcscene%d_shapes' % i] = np.array([len(v), len(f)], dtype=np.int64)
        out['mcscene%d_sha' % i] = np.array(L.digest(v, c, f))
    np.savez_compressed(L.LIVE, **out)
    print('wrote %s: %d arrays, %d bytes' % (L.LIVE, len(out), os.path.getsize(L.LIVE)))


if __name__ == '__main__':
    main()
