"""CPU: the depth-rendering rules of INTEGRATION.md section F as restated in tests/render_ref.py, pinned against the
analytic fp64 ray caster of tests/fusion_ref.py, plus the host pieces of sgnn_amd.render (load_ply, look_at, the
frame table).  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fusion_ref as R  # noqa: E402
import render_ref as RR  # noqa: E402

from sgnn_amd import marching_cubes as mc, render  # noqa: E402

F32 = np.float32
HW = (48, 64)
# |dz| <= g + C_ROUND * z.  About twenty fp32 roundings (2^-24 each) of camera-space values up to ten times z (a 4 m
# room seen from 0.4 m or more) give 1.2e-5, and every sum of rule 7 has non-negative terms, so nothing cancels.
# Largest (|dz| - g) / z seen: -2.4e-5 (room frames), -3.0e-5 (near-plane frames): negative, g alone covers every
# difference found.
C_ROUND = 2e-5
G_SILHOUETTE = 0.01         # g above 1 cm: a silhouette within 1/128 pixel of the centre, left out of the comparison


def analytic(k, pose, hw=HW):
    return R.render(k, pose, hw, R.ROOM_PLANES, R.ROOM_BOXES).astype(np.float64)


def snap_reach(k, pose, hw=HW):
    """(analytic depth, g): g = the largest change of the analytic depth over the probes (i +- 1/128, j +- 1/128),
    what snapping three vertices to 1/256 pixel can move."""
    z = analytic(k, pose, hw)
    g = np.zeros_like(z)
    for du in (-1.0 / 128, 1.0 / 128):
        for dv in (-1.0 / 128, 1.0 / 128):
            kk = np.array([k[0], k[1], k[2] - du, k[3] - dv], np.float64)      # sampling at i + du = shifting cx
            g = np.maximum(g, np.abs(R.render(kk, pose, hw, R.ROOM_PLANES, R.ROOM_BOXES).astype(np.float64) - z))
    return z, g


def compare(got, k, pose, dmin=0.4, dmax=4.0, z_clip=0.1, max_left_out=None):
    """The checks of one frame against the analytic depth; returns the largest (|dz| - g) / z of the compared pixels."""
    z, g = snap_reach(k, pose, got.shape)
    assert np.isfinite(z).all()                                               # a closed room
    bound = g + C_ROUND * z
    left_out = g > G_SILHOUETTE
    if max_left_out is not None:
        assert left_out.mean() <= max_left_out, left_out.mean()
    inside = (z >= dmin + bound) & (z <= dmax - bound)
    assert np.isfinite(got[inside]).all(), 'a hole: %d pixels' % (~np.isfinite(got[inside])).sum()
    # nearer than depth_min blanks the pixel (what lies nearer than z_clip is cut away instead: rule 3)
    outside = ((z < dmin - bound) & (z > z_clip + bound)) | (z > dmax + bound)
    assert (got[outside & ~left_out] == -np.inf).all()
    cmp = inside & ~left_out
    if not cmp.any():
        return 0.0
    dz = np.abs(got[cmp].astype(np.float64) - z[cmp])
    assert (dz <= bound[cmp]).all(), ((dz - g[cmp]) / z[cmp]).max()
    return ((dz - g[cmp]) / z[cmp]).max()


@pytest.mark.parametrize('n', [3, 8])
def test_room_equals_the_analytic_ray_caster(n):
    _, k, poses = R.room_frames(24, HW, seed=1)
    verts, faces = RR.tessellate_room(n)
    got = RR.render_ref(verts, faces, k, poses, HW)
    worst = max(compare(got[f], k[f], poses[f], max_left_out=0.01) for f in range(len(poses)))
    print('tessellation %d: largest (|dz| - g) / z = %.3g (bar %.1g)' % (n, worst, C_ROUND))
    assert np.isfinite(got).mean() > 0.9


def test_no_holes_where_edges_pass_through_pixel_centres():
    # wall at 2 m, fx = 40, 16 x 16 quads of 0.2 m: every vertex column projects onto an integer pixel column
    verts, faces = RR.tessellate_room(16)
    k = np.array([40.0, 40.0, 32.0, 24.0], F32)
    eye = np.array([2.0, 1.6, 1.3])
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1)]
    poses = np.stack([R.look_at(eye, eye + np.array(d, np.float64)) for d in dirs])
    kk = np.tile(k, (len(poses), 1))
    m = RR.camera_rows(poses[0])
    tri = RR.camera_triangles(verts, faces, m, 0.1)
    X, Y, _, _ = RR.screen_triangles(tri, k)
    on_centre = ((X % 256 == 0) & (Y % 256 == 0) & (X >= 0) & (X < 64 * 256) & (Y >= 0) & (Y < 48 * 256)).sum()
    assert on_centre > 100                                                    # the case is what it claims to be
    got = RR.render_ref(verts, faces, kk, poses, (49, 65))
    assert np.isfinite(got).all()
    for f in range(len(poses)):
        compare(got[f], kk[f], poses[f])


def test_face_order_and_winding_change_no_bit():
    rng = np.random.default_rng(3)
    _, k, poses = R.room_frames(4, HW, seed=5)
    for n in (2, 5):
        verts, faces = RR.tessellate_room(n)
        base = RR.render_ref(verts, faces, k, poses, HW)
        assert np.isfinite(base).mean() > 0.9
        shuffled = faces[rng.permutation(len(faces))]
        flip = rng.random(len(faces)) < 0.5
        shuffled[flip] = shuffled[flip][:, ::-1]
        rolled = np.roll(shuffled, 1, axis=1)                                  # and a rotation of every face
        for other in (shuffled, rolled):
            assert np.array_equal(RR.render_ref(verts, other, k, poses, HW).view(np.int32), base.view(np.int32))
    # the clip is exercised: some triangle straddles z_clip and survives
    m = RR.camera_rows(poses[0])
    assert len(RR.camera_triangles(verts, faces, m, 0.1)) > ((RR._transform(m, verts)[faces][:, :, 2] >= 0.1).all(1)).sum()


NEAR_CASES = {
    'wall_5cm': ((0.05, 0.5, 1.3), (0.6, 3.0, 1.2)),            # 5 cm from the wall x = 0, looking along it
    'box_straddles': ((1.85, 1.3, 0.5), (1.6, 0.0, 0.4)),       # the box face x = 1.8 crosses the camera plane
}


@pytest.mark.parametrize('case', sorted(NEAR_CASES))
def test_near_plane(case):
    eye, target = NEAR_CASES[case]
    pose = R.look_at(eye, target)
    k = np.array([0.8 * 64, 0.8 * 64, 31.5, 23.5], F32)
    for n in (1, 4):
        verts, faces = RR.tessellate_room(n)
        m = RR.camera_rows(pose)
        pz = RR._transform(m, verts)[faces][:, :, 2]
        straddle = (pz >= 0.1).any(1) & (pz < 0.1).any(1)
        assert straddle.sum() >= 2                                             # both sides of a shared edge are clipped
        got = RR.render_ref(verts, faces, k[None], pose[None], HW)[0]
        worst = compare(got, k, pose)
        print('%s, tessellation %d: largest (|dz| - g) / z = %.3g' % (case, n, worst))
        z = analytic(k, pose)
        assert ((z > 0.12) & (z < 0.38)).sum() > 20 and (got == -np.inf).sum() > 20   # something is blanked


def test_load_ply_round_trip_and_rejections(tmp_path):
    verts, faces = RR.tessellate_room(3)
    cols = np.random.default_rng(0).integers(0, 255, (len(verts), 3)).astype(np.uint8)
    path = str(tmp_path / 'room.ply')
    mc.save_to_ply(path, torch.from_numpy(verts), torch.from_numpy(cols), torch.from_numpy(faces))
    v, f = render.load_ply(path)
    assert v.dtype == np.float32 and f.dtype == np.int32
    assert np.array_equal(v.view(np.int32), verts.view(np.int32)) and np.array_equal(f, faces)
    blob = open(path, 'rb').read()
    bad = {
        'ascii': (blob.replace(b'format binary_little_endian 1.0', b'format ascii 1.0'), 'format ascii'),
        'big': (blob.replace(b'binary_little_endian', b'binary_big_endian'), 'binary_big_endian'),
        'strips': (blob.replace(b'property list uchar int vertex_indices', b'property list uchar float vertex_indices'),
                   'property list uchar float'),
    }
    for name, (data, needle) in bad.items():
        p = str(tmp_path / (name + '.ply'))
        open(p, 'wb').write(data)
        with pytest.raises(ValueError, match=needle):
            render.load_ply(p)
    head, body = blob.split(b'end_header\n')
    quad = bytearray(body)
    quad[len(verts) * 15] = 4                                                  # the first face claims four vertices
    p = str(tmp_path / 'quad.ply')
    open(p, 'wb').write(head + b'end_header\n' + bytes(quad))
    with pytest.raises(ValueError, match='triangles only'):
        render.load_ply(p)


def test_look_at_and_frame_table_follow_the_restatement():
    _, k, poses = R.room_frames(7, HW, seed=2)
    rng = np.random.default_rng(1)
    eyes = rng.uniform(0.5, 2.0, (9, 3))
    targets = eyes + rng.normal(size=(9, 3))
    targets[4] = eyes[4] + (0.0, 0.0, -1.0)                                    # straight down: the fallback axis
    got = render.look_at(eyes, targets)
    assert got.shape == (9, 4, 4)
    for i in range(9):
        assert np.array_equal(got[i], R.look_at(eyes[i], targets[i]))
    assert np.array_equal(render.look_at(eyes[0], targets[0]), got[0])
    poses[3, 0, 0] = np.nan
    t = render.frame_table(k, poses)
    assert t.dtype.itemsize == 64 and np.isnan(t['m'][3]).all()
    for f in (0, 6):
        assert np.array_equal(t['m'][f].reshape(3, 4), RR.camera_rows(poses[f]))
    assert np.array_equal(t['intr'], k)
    with pytest.raises(ValueError):
        render.frame_table(k[:3], poses)


def _distance_to_planes(p):
    """Distance of points (n, 3) to the nearest of the room's six planes."""
    return np.min([np.abs(p @ np.asarray(nrm, np.float64) - c) for nrm, c in R.ROOM_PLANES], 0)


def test_fused_rendered_frames_put_the_zero_crossing_on_the_planes():
    vs = 0.1
    _, k, poses = R.room_frames(24, HW, seed=1)
    # the empty room: behind a box a projective TSDF changes sign away from any surface, whatever made the frames
    verts, faces = RR.box_mesh((0.0, 0.0, 0.0), (4.0, 3.2, 2.6), 4)
    depth = RR.render_ref(verts.astype(F32), faces, k, poses, HW)
    origin = np.array([-0.35, -0.35, -0.35])
    w2g = R.grid_transform(origin, vs)
    grid = R.Grid((47, 39, 33), vs, w2g).integrate(depth, k, poses)
    s = grid.sdf.astype(np.float64)                                            # (z, y, x)
    worst, crossings = 0.0, 0
    for ax in range(3):
        a = np.moveaxis(s, ax, 0)
        s0, s1 = a[:-1], a[1:]
        with np.errstate(invalid='ignore'):
            flip = np.isfinite(s0) & np.isfinite(s1) & ((s0 > 0) != (s1 > 0)) & (s0 != s1)
        idx = np.stack(np.nonzero(flip), 1).astype(np.float64)
        idx[:, 0] += (s0[flip] / (s0[flip] - s1[flip]))                        # linear interpolation to sdf = 0
        zyx = np.empty_like(idx)
        order = [ax] + [i for i in range(3) if i != ax]
        for col, dim in enumerate(order):
            zyx[:, dim] = idx[:, col]
        world = zyx[:, ::-1] * vs + origin
        d = _distance_to_planes(world)
        crossings += len(d)
        worst = max(worst, d.max() / vs)
    print('zero crossings: %d, largest distance from its plane: %.3f voxels' % (crossings, worst))
    assert crossings > 1000
    assert worst < 1.0              # measured 0.20 voxels; above one voxel rule 4's pixel convention would be wrong
