"""GPU: the sensor kernels (sgnn_amd.sensor, csrc/sensor.hip) against the NumPy restatement of tests/sensor_ref.py:
every mask and every depth bit for bit, -inf included; the carry of the shadow scan, its mirror property, determinism,
the invariants of the output and the statistics of the axial noise."""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sensor_ref as R  # noqa: E402

from sgnn_amd import sensor  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def bits(a):
    a = a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a, F32).view(np.uint32)


def device_model(m):
    return sensor.SensorModel(**{k: float(v) for k, v in m.items()})


@functools.lru_cache(maxsize=None)
def scene(name, shape):
    depth, K = R.SCENES[name](*shape)
    depth.setflags(write=False)
    return depth, K


@pytest.mark.parametrize('shape', R.SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
@pytest.mark.parametrize('name', sorted(R.SCENES))
def test_every_setting_matches_the_restatement_bit_for_bit(name, shape):
    depth, K = scene(name, shape)
    dev = torch.tensor(depth, device='cuda')
    for setting, (base, changes) in R.SETTINGS.items():
        m = R.model(base, **changes)
        want = R.degrade(depth, K, m, seed=3)
        got = sensor.degrade(dev, K, device_model(m), seed=3)
        assert got.shape == depth.shape and got.dtype == torch.float32 and got.is_cuda
        assert np.array_equal(bits(got), bits(want)), (setting, int((bits(got) != bits(want)).sum()))
        if setting == 'off':
            assert np.array_equal(bits(got), bits(depth))
    # one set of intrinsics per frame
    Kf = R.per_frame_cameras(shape[0], shape[1], shape[2])
    for base, changes in (R.SETTINGS['all'], R.SETTINGS['all_left']):
        m = R.model(base, **changes)
        got = sensor.degrade(dev, torch.from_numpy(Kf).cuda(), device_model(m), seed=8)
        assert np.array_equal(bits(got), bits(R.degrade(depth, Kf, m, seed=8)))
    for baseline in (0.075, -0.075, 0.0, 0.5):
        got = sensor.shadow_mask(dev, Kf, baseline)
        assert got.dtype == torch.bool and np.array_equal(got.cpu().numpy(), R.shadow_mask(depth, Kf, baseline))


def test_the_cases_exercise_every_stage():
    """The bit-for-bit cases mean something: on the largest shape every stage removes or moves pixels."""
    depth, K = scene('box', (2, 33, 70))
    lost = {}
    R.degrade(depth, K, R.model(R.DEFAULTS, drop=0.2), seed=3, stages=lost)
    assert all(lost[k].sum() > 0 for k in ('outside', 'range', 'shadow', 'edge', 'grazing', 'dropout')), lost.keys()
    assert R.shadow_mask(depth, R.intrinsics(K, 2), -0.075).sum() > 0


def test_a_single_frame_and_host_arrays():
    depth, K = scene('box', (2, 33, 70))
    m = R.model()
    got = sensor.degrade(depth[1], K, device_model(m), seed=3, frame_ids=[1])
    assert got.shape == (33, 70) and np.array_equal(bits(got), bits(R.degrade(depth, K, m, seed=3)[1]))
    mask = sensor.shadow_mask(depth[0], K)
    assert mask.shape == (33, 70) and np.array_equal(mask.cpu().numpy(), R.shadow_mask(depth[:1], R.intrinsics(K, 1), 0.075)[0])
    empty = sensor.degrade(np.zeros((0, 4, 5), F32), K)
    assert empty.shape == (0, 4, 5) and sensor.shadow_mask(np.zeros((2, 0, 5), F32), K).shape == (2, 0, 5)
    for bad in (dict(depth=depth[0, 0]), dict(intrinsics=np.ones((3, 4), F32)), dict(intrinsics=[0.0, 50.0, 1.0, 1.0]),
                dict(frame_ids=[0]), dict(frame_ids=[0, -1]), dict(seed=-1), dict(model='kinect')):
        args = dict(dict(depth=depth, intrinsics=K), **bad)
        with pytest.raises(ValueError):
            sensor.degrade(**args)


def test_the_shadow_carries_from_the_last_chunk_to_the_first():
    row = np.full(130, 3.0, F32)
    row[129] = 0.5                                                  # the only occluder: the last pixel, chunk 2
    K = np.array([570.0, 570.0, 64.5, 0.0], F32)                    # its u = 129 - 85.5 = 43.5; the wall's u = x - 14.25
    want = R.shadow_row_scan(row, K[0], 0.075)
    assert np.array_equal(np.nonzero(want)[0], np.arange(58, 129)) and want[:64].any()
    got = sensor.shadow_mask(row.reshape(1, 1, 130), K, 0.075)
    assert np.array_equal(got.cpu().numpy().reshape(-1), want)
    # and in the other direction: the only occluder is pixel 0 of chunk 0, the shadow reaches chunk 1
    row = row[::-1].copy()
    want = R.shadow_row_scan(row, K[0], -0.075)
    assert np.array_equal(np.nonzero(want)[0], np.arange(1, 72))
    got = sensor.shadow_mask(row.reshape(1, 1, 130), K, -0.075)
    assert np.array_equal(got.cpu().numpy().reshape(-1), want)
    # nine rows in one call (three blocks), each with its own occluder: the rows do not talk to each other
    rows = np.full((1, 9, 130), 3.0, F32)
    for y in range(9):
        rows[0, y, 129 - 13 * y] = 0.5
    got = sensor.shadow_mask(rows, K, 0.075)
    assert np.array_equal(got.cpu().numpy(), R.shadow_mask(rows, R.intrinsics(K, 1), 0.075)) and got[0, :, :64].any()


def test_the_mirrored_frame_has_the_mirrored_shadow():
    depth, K = scene('box', (2, 33, 70))
    w = depth.shape[2]
    Km = K.copy()
    Km[2] = F32(w - 1) - K[2]
    assert F32(w - 1) - Km[2] == K[2]                               # the mirrored cx is exact here; u does not read it anyway
    mirrored = np.ascontiguousarray(depth[:, :, ::-1])
    for baseline in (0.075, -0.075):
        a = sensor.shadow_mask(depth, K, baseline).cpu().numpy()
        b = sensor.shadow_mask(mirrored, Km, -baseline).cpu().numpy()
        assert a.any() and np.array_equal(b, a[:, :, ::-1])


def test_the_result_depends_on_the_seed_and_on_nothing_else():
    depth, K = scene('box', (3, 5, 7))
    big, Kb = scene('box', (2, 33, 70))
    m = sensor.SensorModel()
    for d, k in ((depth, K), (np.concatenate([big, big[:1]]), Kb)):
        dev = torch.from_numpy(d).cuda()
        whole = sensor.degrade(dev, k, m, seed=4)
        assert np.array_equal(bits(whole), bits(sensor.degrade(dev, k, m, seed=4)))
        assert not np.array_equal(bits(whole), bits(sensor.degrade(dev, k, m, seed=5)))
        parts = [sensor.degrade(dev[0:2], k, m, seed=4, frame_ids=[0, 1]),
                 sensor.degrade(dev[2:3], k, m, seed=4, frame_ids=torch.tensor([2]))]
        assert np.array_equal(bits(torch.cat(parts)), bits(whole))
    far = sensor.degrade(dev[:1], k, m, seed=(1 << 64) - 1, frame_ids=[1 << 40])     # wrap-around arithmetic
    assert np.array_equal(bits(far), bits(R.degrade(big[:1], Kb, R.model(), seed=(1 << 64) - 1, frame_ids=[1 << 40])))


def test_invariants_of_the_output():
    depth, K = scene('box', (2, 33, 70))
    hole = ~np.isfinite(depth)
    m = sensor.SensorModel(lateral_sigma=0.0)
    out = sensor.degrade(depth, K, m, seed=6).cpu().numpy()
    assert hole.any() and (out[hole] == -np.inf).all()
    for model in (m, sensor.SensorModel(), sensor.SensorModel(baseline=-0.075)):
        out = sensor.degrade(depth, K, model, seed=6).cpu().numpy()
        live = np.isfinite(out)
        assert live.sum() > 1000 and (out[live] > 0).all() and (out[~live] == -np.inf).all()
        # B / z is a multiple of q to within one ulp of the division z2 = B / dq (fp32: 2^-23 relative)
        B = np.float64(F32(K[0]) * F32(0.075))
        steps = B / out[live].astype(np.float64) / 0.125
        assert np.abs(steps - np.round(steps)).max() <= np.round(steps).max() * 2.0 ** -23


@pytest.mark.parametrize('kind', ['fit', 'constant'])
def test_the_axial_noise_has_the_sigma_of_the_rule(kind):
    depth = np.full((1, 64, 64), 2.0, F32)
    K = np.array([60.0, 60.0, 31.5, 31.5], F32)
    off = sensor.SensorModel.off()
    if kind == 'fit':
        m = off._replace(a0=0.0012, a1=0.0019, a2=0.4, a3=0.05)
        sigma = 0.0012 + 0.0019 * (2.0 - 0.4) ** 2
    else:
        c = sensor.SensorModel.constant(0.01)
        m = off._replace(a0=c.a0, a1=c.a1, a2=c.a2, a3=c.a3)
        sigma = 0.01
    out = sensor.degrade(depth, K, m, seed=12).cpu().numpy().astype(np.float64)[0]
    inner = out[1:-1, 1:-1].ravel() - 2.0                           # fronto-parallel: tan^2 = 0 up to rounding
    n = inner.size
    assert np.isfinite(out).all() and n == 62 * 62
    print('sensor noise %s: sigma %.6g, std %.6g, mean %.3g, n %d' % (kind, sigma, inner.std(ddof=1), inner.mean(), n))
    assert abs(inner.std(ddof=1) - sigma) <= 5 * sigma / math.sqrt(2 * n)
    assert abs(inner.mean()) <= 5 * sigma / math.sqrt(n)


def test_end_to_end_room_printed_not_asserted(capsys):
    """The room of tests/points_scenes.py rendered, degraded and fused: the share of pixels each stage takes and the
    RMS difference of the fused sdf against the clean fusion inside the band.  Observations for INTEGRATION.md
    section V; nothing here is asserted but that the chain runs."""
    import points_scenes as PS
    from sgnn_amd import fusion, render
    room = PS.room()
    k, poses = room['k'], room['poses']
    depth = render.render_depth(room['verts'], room['faces'], k, poses, PS.ROOM_HW)
    noisy = sensor.degrade(depth, k, sensor.SensorModel(), seed=0)
    lost = {}
    ref = R.degrade(depth.cpu().numpy(), k, R.model(), seed=0, stages=lost)
    seen = int(np.isfinite(depth.cpu().numpy()).sum())
    shares = {name: round(float(v.sum()) / depth.numel(), 4) for name, v in lost.items()}
    clean = fusion.TSDFVolume(room['dims'], PS.VS, room['w2g']).integrate(depth, k, poses)
    rough = fusion.TSDFVolume(room['dims'], PS.VS, room['w2g']).integrate(noisy, k, poses)
    a, b = clean.sdf().cpu().numpy().astype(np.float64), rough.sdf().cpu().numpy().astype(np.float64)
    with np.errstate(invalid='ignore'):
        both = np.isfinite(a) & np.isfinite(b) & (np.abs(a) < 3 * float(PS.VS))
    rms = float(np.sqrt(np.mean((a[both] - b[both]) ** 2))) if both.any() else float('nan')
    with capsys.disabled():
        print('\nsensor end to end: %d of %d pixels seen, %d after degrade; lost per stage %s; fused sdf rms %.5f m '
              'over %d band voxels (voxel %.3f m); known voxels %d clean, %d degraded' % (
                  seen, depth.numel(), int(torch.isfinite(noisy).sum()), shares, rms, int(both.sum()), float(PS.VS),
                  int(np.isfinite(a).sum()), int(np.isfinite(b).sum())))
    assert np.array_equal(bits(noisy), bits(ref))
