"""Training chunks cut from a fused scan pair on the GPU: TSDFVolume input + TSDFPyramid target -> the collated
batch train.GraphStep / train.train_step consume, or .sdfs files (rules in INTEGRATION.md "Training chunks").

The reference trains on .sdfs chunks that a tool it never shipped cut from its scans; here the crops come straight
from the device volumes of sgnn_amd.fusion (kernels: sgnn_amd/csrc/chunks.hip):

    target = fusion.TSDFPyramid((dx, dy, dz), 0.02, world2grid).integrate(depth[::3], K[::3], pose[::3])
    scan = target[0].copy()                                      # the input: a subset of the frames
    target.integrate(rest_depth, rest_K, rest_pose)              # the target: all of them, at four voxel sizes
    cutter = chunks.ChunkCutter(scan, target, crop_zyx=(128, 64, 64), stride_zyx=(128, 32, 32))
    cand = cutter.candidates(min_target=4000, min_input=1000)    # windows worth training on, raster order
    batch = cutter.batch(cand.origins[perm[:8]])                 # what DeviceBatchLoader yields in chunk mode
    loss = graph_step(batch, loss_weights)
    cutter.save(cand.origins, out_dir, 'scene0000_00')           # the same crops as .sdfs files

Which windows to train on, and in what order, is the caller's choice: nothing here draws random numbers.
"""
import collections
import os

import numpy as np
import torch

from . import _glue, _lib, data

BRICK = 8            # scoring granularity of sgnn_chunk_score: window origins, strides and extents are multiples of it
LEVELS = 4           # a .sdfs chunk carries the target at 1x and three hierarchy blocks (1/2, 1/4, 1/8)

Candidates = collections.namedtuple('Candidates', ['origins', 'n_target', 'n_input'])


def _triple(v, what):
    t = tuple(int(x) for x in v)
    if len(t) != 3 or any(int(x) != x for x in v):
        raise ValueError('%s must be three integers (z, y, x), got %r' % (what, v))
    return t


class ChunkCutter(object):
    """Windows of `crop_zyx` voxels over an input volume and its target pyramid.

    input_volume: fusion.TSDFVolume with the dims, voxel size and world2grid of target_pyramid[0];
    target_pyramid: fusion.TSDFPyramid with 4 levels (the .sdfs layout: target + hierarchy 1/2, 1/4, 1/8).
    crop_zyx: multiples of 4 * 2**(levels-1) = 32 (data._padded_dims); stride_zyx and every origin: multiples of
    2**(levels-1) = 8, so that a crop's coarse windows start on whole voxels.  truncation: the loaders'
    |sdf / voxel_size| < truncation input filter; trunc_factor: the files' |sdf| <= trunc_factor * voxel_size band
    (per level: its own voxel size).  A window may reach past the volume: out there the input has no sites, targets
    are -inf and known is 255."""

    def __init__(self, input_volume, target_pyramid, crop_zyx=(128, 64, 64), stride_zyx=(128, 32, 32), truncation=3.0,
                 trunc_factor=6.0):
        _lib.require_gpu()
        if len(target_pyramid) != LEVELS:
            raise ValueError('a training chunk stores %d target levels, the pyramid has %d' % (LEVELS,
                                                                                             len(target_pyramid)))
        fine = target_pyramid[0]
        if tuple(input_volume.dims_xyz) != tuple(fine.dims_xyz):
            raise ValueError('input volume is %s voxels, the target %s' % (input_volume.dims_xyz, fine.dims_xyz))
        if np.float32(input_volume.voxel_size) != np.float32(fine.voxel_size):
            raise ValueError('input voxel size %r differs from the target\'s %r' % (input_volume.voxel_size,
                                                                                   fine.voxel_size))
        if not np.array_equal(input_volume.world2grid, fine.world2grid):
            raise ValueError('input and target volumes have different world2grid matrices')
        if input_volume.device != fine.device:
            raise ValueError('input and target volumes live on different devices')
        for k in range(1, LEVELS):
            want = tuple(-(-d // 2 ** k) for d in fine.dims_xyz)
            if tuple(target_pyramid[k].dims_xyz) != want:
                raise ValueError('pyramid level %d is %s voxels, expected %s' % (k, target_pyramid[k].dims_xyz, want))
        self.crop = _triple(crop_zyx, 'crop_zyx')
        self.stride = _triple(stride_zyx, 'stride_zyx')
        q = 4 * 2 ** (LEVELS - 1)
        if any(c < q or c % q for c in self.crop):
            raise ValueError('crop_zyx %s: every entry must be a positive multiple of %d' % (self.crop, q))
        if any(s < BRICK or s % BRICK for s in self.stride):
            raise ValueError('stride_zyx %s: every entry must be a positive multiple of %d' % (self.stride, BRICK))
        self.input, self.target, self.device = input_volume, target_pyramid, fine.device
        self.voxel_size = np.float32(fine.voxel_size)
        self.truncation, self.trunc_factor = np.float32(truncation), np.float32(trunc_factor)
        # windows per axis: enough to cover the volume, the last one may overhang
        self.grid = tuple(-(-max(d - c, 0) // s) + 1 for d, c, s in zip(fine.dims_zyx, self.crop, self.stride))

    def _keep(self, level):
        return float(self.trunc_factor * np.float32(self.target[level].voxel_size))

    # ---- scoring ----
    def scores(self):
        """(origins (W, 3) int64 z, y, x; counts (W, 2) int64 n_target, n_input) of every window of the stride grid,
        raster order.  n_target: voxels with |sdf_target / vs| < truncation; n_input: voxels with |sdf_input| <=
        trunc_factor * vs and |sdf_input / vs| < truncation.  One pass over the two fine volumes; the table (a few
        thousand entries) is read back once."""
        dx, dy, dz = self.target[0].dims_xyz
        nwz, nwy, nwx = self.grid
        nbricks = -(-dz // BRICK) * -(-dy // BRICK) * -(-dx // BRICK)
        bricks = torch.empty((nbricks, 2), dtype=torch.int32, device=self.device)
        table = torch.empty((nwz * nwy * nwx, 2), dtype=torch.int32, device=self.device)
        _lib.call('sgnn_chunk_score', self.target[0].sdf().data_ptr(), self.input.sdf().data_ptr(), dx, dy, dz,
                  float(self.voxel_size), float(self.truncation), self._keep(0), *self.crop, *self.stride, nwz, nwy, nwx,
                  bricks.data_ptr(), table.data_ptr())
        w = np.stack(np.meshgrid(np.arange(nwz), np.arange(nwy), np.arange(nwx), indexing='ij'), -1).reshape(-1, 3)
        return w.astype(np.int64) * np.array(self.stride, dtype=np.int64), table.cpu().numpy().astype(np.int64)

    def candidates(self, min_target=1, min_input=1):
        """Candidates(origins (M, 3) int64 z, y, x; n_target (M,); n_input (M,)), host arrays: the windows with
        n_target >= min_target and n_input >= min_input, in raster order of the origin."""
        origins, counts = self.scores()
        ok = (counts[:, 0] >= min_target) & (counts[:, 1] >= min_input)
        return Candidates(origins[ok], counts[ok, 0], counts[ok, 1])

    # ---- extraction ----
    def _origins(self, origins):
        o = np.asarray(origins)
        if o.size == 0:
            raise ValueError('no origins given')
        if o.ndim != 2 or o.shape[1] != 3 or not np.issubdtype(o.dtype, np.integer):
            raise ValueError('origins must be an integer array of shape (B, 3) (z, y, x), got %s %s' % (o.dtype, o.shape))
        o = o.astype(np.int64)
        if (o % BRICK).any() or (o < 0).any() or (o >= 2 ** 30).any():
            raise ValueError('every origin must be a non-negative multiple of %d' % BRICK)
        if o.shape[0] * int(np.prod(self.crop)) >= 2 ** 31:
            raise ValueError('%d crops of %s voxels exceed one batch (2^31 voxels)' % (o.shape[0], self.crop))
        return o, torch.from_numpy(o.astype(np.int32)).to(self.device)

    def _dense(self, volume, level, dev_origins, nb, divisor, known=False):
        """(nb, 1, Z/f, Y/f, X/f) fp32 of one volume: (sdf / f) / divisor inside the level's band, else -inf; one
        launch for all crops.  With known also the (nb, 1, Z, Y, X) u8 codes."""
        f = 2 ** level
        cz, cy, cx = (c // f for c in self.crop)
        dx, dy, dz = volume.dims_xyz
        out = torch.empty((nb, 1, cz, cy, cx), dtype=torch.float32, device=self.device)
        kn = torch.empty((nb, 1, cz, cy, cx), dtype=torch.uint8, device=self.device) if known else None
        keep = float(self.trunc_factor * np.float32(volume.voxel_size))
        _lib.call('sgnn_chunk_crop', volume.sdf().data_ptr(), dx, dy, dz, dev_origins.data_ptr(), nb, cz, cy, cx, level,
                  keep, float(divisor), out.data_ptr(), _lib.ptr(kn))
        return (out, kn) if known else out

    def _world2grid(self, o):
        w = np.repeat(self.target[0].world2grid[None], len(o), 0).astype(np.float32)
        w[:, :3, 3] -= o[:, ::-1].astype(np.float32)               # rows x, y, z; one fp32 subtraction each
        return w

    def names(self, origins, prefix='chunk'):
        return ['%s_z%d_y%d_x%d' % (prefix, z, y, x) for z, y, x in np.asarray(origins).reshape(-1, 3)]

    def batch(self, origins, prefix='chunk'):
        """The collated device batch of the crops at `origins` ((B, 3) z, y, x), key for key what DeviceBatchLoader
        yields in chunk mode for the files save() writes: name, input [locs (n, 4) int64 z, y, x, b relative to the
        crop; feats (n, 1) sdf / vs], sdf (B, 1, Z, Y, X), known (B, 1, Z, Y, X) u8, hierarchy [1/8, 1/4, 1/2],
        world2grid (B, 4, 4), orig_dims (B, 3).  The row count is the only value read back."""
        o, dev_o = self._origins(origins)
        nb = o.shape[0]
        cz, cy, cx = self.crop
        vol, vs, dev = self.input, float(self.voxel_size), self.device
        dx, dy, dz = vol.dims_xyz
        n = nb * cz * cy * cx
        # sparse input: flag -> stable compaction -> rows (as TSDFVolume._compact / scan_sample)
        mask = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.call('sgnn_chunk_flag', vol.sdf().data_ptr(), dx, dy, dz, dev_o.data_ptr(), nb, cz, cy, cx, self._keep(0),
                  float(self.truncation), vs, mask.data_ptr())
        sel, count = _glue.compact(mask, n, dev, read=False)
        # dense targets while the count travels: one launch per level
        sdf, known = self._dense(self.target[0], 0, dev_o, nb, vs, known=True)
        hierarchy = [self._dense(self.target[k], k, dev_o, nb, vs) for k in (3, 2, 1)]
        m = int(count.item())
        locs = torch.empty((max(m, 1), 4), dtype=torch.int64, device=dev)
        feats = torch.empty((max(m, 1), 1), dtype=torch.float32, device=dev)
        _lib.call('sgnn_chunk_emit_rows', vol.sdf().data_ptr(), dx, dy, dz, dev_o.data_ptr(), nb, cz, cy, cx, vs,
                  sel.data_ptr(), count.data_ptr(), m, locs.data_ptr(), feats.data_ptr())
        return {'name': self.names(o, prefix), 'input': [locs[:m], feats[:m]], 'sdf': sdf,
                'world2grid': torch.from_numpy(self._world2grid(o)).to(dev), 'known': known, 'hierarchy': hierarchy,
                'orig_dims': torch.tensor([[cz, cy, cx]] * nb, dtype=torch.long)}

    def save(self, origins, out_dir, prefix='chunk'):
        """One .sdfs per crop (data.write_train_file), named as batch() names them; returns the paths.  The blocks
        hold the volumes' metric values inside their bands (input and target: |sdf| <= trunc_factor * vs; hierarchy
        level f: sdf_f / f where |sdf_f| <= trunc_factor * f * vs), raster order; the loaders' truncation filter is
        not applied to a file.  The crops are cut on the device (divisor 1 keeps metres) and cross to the host."""
        o, dev_o = self._origins(origins)
        nb = o.shape[0]
        inp = self._dense(self.input, 0, dev_o, nb, 1.0).cpu().numpy()[:, 0]
        tgt = self._dense(self.target[0], 0, dev_o, nb, 1.0).cpu().numpy()[:, 0]
        known = self._dense(self.target[0], 0, dev_o, nb, float(self.voxel_size), known=True)[1].cpu().numpy()[:, 0]
        hier = [self._dense(self.target[k], k, dev_o, nb, 1.0).cpu().numpy()[:, 0] for k in (1, 2, 3)]
        w2g = self._world2grid(o)

        def block(dense):
            z, y, x = np.nonzero(np.isfinite(dense))
            return np.stack([z, y, x], 1), dense[z, y, x]

        paths = []
        for b, name in enumerate(self.names(o, prefix)):
            paths.append(os.path.join(str(out_dir), name + '.sdfs'))
            data.write_train_file(paths[-1], self.crop, self.voxel_size, w2g[b], block(inp[b]), block(tgt[b]), known[b],
                                  [block(h[b]) for h in hier])
        return paths
