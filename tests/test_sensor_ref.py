"""Host: the NumPy restatement of INTEGRATION.md section V (tests/sensor_ref.py) against the definitions read
literally, and the host half of sgnn_amd.sensor (SensorModel, keep_frames, hash64).  No GPU."""
import math
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import sensor_ref as R  # noqa: E402

F32 = np.float32


def random_row(rng, w, kind):
    if kind == 'invalid':
        return rng.choice(np.array([-np.inf, np.nan, 0.0, -1.0, np.inf], F32), size=w)
    row = rng.uniform(0.5, 4.0, size=w).astype(F32)
    if kind == 'steps':                                             # a few fronto-parallel surfaces: ties in u are likely
        row = rng.choice(np.array([0.75, 1.5, 3.0], F32), size=w)
    row[rng.random(w) < 0.2] = -np.inf
    return row


@pytest.mark.parametrize('baseline', [0.075, -0.075, 0.0, 1.0])
def test_the_scan_form_of_the_shadow_is_its_definition(baseline):
    rng = np.random.default_rng(11)
    shadows = 0
    for w in (1, 2, 3, 17, 64, 65, 130):
        for kind in ('invalid', 'random', 'steps'):
            for fx in (60.0, 570.0):
                row = random_row(rng, w, kind)
                want = R.shadow_row_literal(row, fx, baseline)
                assert np.array_equal(R.shadow_row_scan(row, fx, baseline), want), (w, kind, fx)
                assert not want.any() or (kind != 'invalid' and w > 1 and baseline != 0)
                shadows += int(want.sum())
    assert (shadows > 0) == (baseline != 0)


def test_a_nearer_surface_on_the_right_shadows_its_left_neighbour():
    row = np.full(40, 2.0, F32)
    row[20:30] = 1.0                                                # disparity 570 * 0.075 (1 - 1/2) = 21.4 pixels
    got = R.shadow_row_scan(row, 570.0, 0.075)
    assert np.array_equal(np.nonzero(got)[0], np.arange(0, 20))     # u of x = 20 is -22.75, below that of every x < 20
    row[:] = 2.0
    row[20:22] = 1.0
    assert np.array_equal(np.nonzero(R.shadow_row_scan(row, 570.0, 0.075))[0], np.arange(0, 20))
    assert np.array_equal(np.nonzero(R.shadow_row_scan(row, 570.0, -0.075))[0], np.arange(22, 40))
    assert np.array_equal(np.nonzero(R.shadow_row_scan(row, 57.0, 0.075))[0], np.arange(18, 20))


def test_the_irwin_hall_integers_have_the_exact_mean_and_unit_variance():
    n = 1 << 16
    r = R.draws(5, [0, 1, 2, 3], 128, 128)                          # 4 streams of 2^16 pixels
    # the centring constants are the exact means of the sums of fields uniform on 0 .. 2^b - 1, and integers
    assert 8 * 65535 == 2 * 262140 and 4 * 255 == 2 * 510
    # the scales are the fp32 roundings of 1 / sqrt(n (2^2b - 1) / 12)
    assert R.C8 == F32(1.0 / math.sqrt(8 * (65536.0 ** 2 - 1) / 12)) and R.C4 == F32(1.0 / math.sqrt(4 * (256.0 ** 2 - 1) / 12))
    samples = {8: R.gauss8(r[0], r[1]).ravel(), 4: np.concatenate([R.gauss4(r[2] & np.uint64(0xffffffff)).ravel()[:n // 2],
                                                                  R.gauss4(r[2] >> np.uint64(32)).ravel()[:n // 2]])}
    for fields, g in samples.items():
        assert g.dtype == F32 and g.size == n
        g = g.astype(np.float64)
        # a sum of `fields` uniforms has excess kurtosis -1.2 / fields: var(s^2) = (2 - 1.2 / fields) / n
        se_var = math.sqrt((2.0 - 1.2 / fields) / n)
        assert abs(g.mean()) <= 5.0 / math.sqrt(n), (fields, g.mean())
        assert abs(g.var() - 1.0) <= 5.0 * se_var, (fields, g.var())
        bound = (4.9, 3.5)[fields == 4]
        assert np.abs(g).max() <= bound
    assert abs(262140 * float(R.C8) - 4.8989) < 1e-4 and abs(510 * float(R.C4) - 3.4506) < 1e-4   # where the tails end


def test_round_half_away():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999997, -0.49999997, 8388609.0, -3.2, 0.0, np.inf, np.nan], F32)
    want = np.array([1, -1, 2, -2, 3, 0, 0, 8388609.0, -3, 0, np.inf, np.nan], F32)
    assert np.array_equal(R.round_away(v), want, equal_nan=True)


@pytest.mark.parametrize('scene', sorted(R.SCENES))
def test_every_stage_off_returns_the_input(scene):
    for shape in R.SHAPES:
        depth, K = R.SCENES[scene](*shape)
        out = R.degrade(depth, K, R.model(R.OFF), seed=9)
        assert np.array_equal(out.view(np.uint32), depth.view(np.uint32))
    assert not np.isfinite(R.SCENES['box'](2, 33, 70)[0]).all()


def test_each_stage_removes_what_it_names():
    depth, K = R.box_scene(2, 33, 70)
    for name, expect in (('jitter', 'outside'), ('range', 'range'), ('shadow', 'shadow'), ('shadow_left', 'shadow'),
                         ('edges', 'edge'), ('grazing', 'grazing'), ('dropout', 'dropout')):
        base, changes = R.SETTINGS[name]
        lost = {}
        out = R.degrade(depth, K, R.model(base, **changes), seed=2, stages=lost)
        holes = int((~np.isfinite(depth)).sum())
        assert lost[expect].sum() > (holes if expect == 'range' else 0), name
        assert np.isfinite(out).sum() < np.isfinite(depth).sum()
    # on the plane alone (across the box's silhouette tan^2 has no bound): |noise| <= 4.9 sigma, with z < 3.3 and
    # tan^2 < 1 sigma < (0.0012 + 0.0019 * 2.9^2) * 1.05 = 0.018; the disparity moves by at most half a quantum
    depth, K = R.plane_scene(2, 33, 70)
    assert depth.max() < 3.3
    out = R.degrade(depth, K, R.model(R.SETTINGS['noise'][0], **R.SETTINGS['noise'][1]), seed=2)
    assert np.isfinite(out).all() and (out != depth).mean() > 0.9 and np.abs(out - depth).max() < 4.9 * 0.018
    out = R.degrade(depth, K, R.model(R.OFF, baseline=0.075, disparity_quantum=0.125), seed=2).astype(np.float64)
    B = float(K[0]) * 0.075
    assert np.isfinite(out).all() and np.abs(B / out - B / depth).max() <= 0.0625 * (1 + 1e-5)
    steps = B / out / 0.125
    assert np.abs(steps - np.round(steps)).max() < 1e-5 and len(np.unique(np.round(steps))) > 5


def test_frames_split_over_calls_give_the_bits_of_the_whole_call():
    depth, K = R.box_scene(3, 9, 20)
    m = R.model()
    whole = R.degrade(depth, K, m, seed=4)
    parts = [R.degrade(depth[0:2], K, m, seed=4, frame_ids=[0, 1]), R.degrade(depth[2:3], K, m, seed=4, frame_ids=[2])]
    assert np.array_equal(np.concatenate(parts).view(np.uint32), whole.view(np.uint32))
    assert not np.array_equal(R.degrade(depth, K, m, seed=5).view(np.uint32), whole.view(np.uint32))


def test_hash64_is_the_library_hash():
    from sgnn_amd import sensor
    for k in (0, 1, 12345, (1 << 64) - 1, 0x9e3779b97f4a7c15):
        assert sensor.hash64(k) == int(R.hash64(np.uint64(k)))
    assert sensor.hash64(1) == 0xb456bcfc34c2cb2c                   # murmur3 fmix64(1)


def test_keep_frames():
    from sgnn_amd import sensor
    n = 1000
    draws = R.frame_draws(n, 7)
    assert draws.min() > 0 and draws.max() < 1
    for chance in (0.0, 0.25, 0.65, 1.0):
        keep = sensor.keep_frames(n, chance, seed=7)
        assert keep.dtype == np.int64 and np.array_equal(keep, np.nonzero(draws > chance)[0])
        assert np.array_equal(keep, sensor.keep_frames(n, chance, seed=7))
        assert np.array_equal(keep, R.keep_frames(n, chance, 7))
    assert np.array_equal(sensor.keep_frames(n, 0.0), np.arange(n)) and sensor.keep_frames(n, 1.0).size == 0
    kept = sensor.keep_frames(n)                                    # a binomial share: 5 standard deviations
    assert abs(kept.size - 0.35 * n) <= 5 * math.sqrt(n * 0.35 * 0.65)
    assert not np.array_equal(kept, sensor.keep_frames(n, seed=1))
    assert np.array_equal(sensor.keep_frames(10, 0.65, seed=7), keep_prefix(sensor.keep_frames(n, 0.65, seed=7), 10))
    assert sensor.keep_frames(0).size == 0
    for bad in (dict(n=-1), dict(n=3, chance_drop=1.5), dict(n=3, chance_drop=float('nan')), dict(n=3, seed=-1)):
        with pytest.raises(ValueError):
            sensor.keep_frames(**bad)


def keep_prefix(keep, n):
    return keep[keep < n]


def test_sensor_model():
    from sgnn_amd import sensor
    m = sensor.SensorModel()
    assert m._fields == R.FIELDS == sensor.MODEL_DTYPE.names
    assert all(F32(getattr(m, k)) == F32(R.DEFAULTS[k]) for k in R.FIELDS)
    assert F32(m.cos_min) == F32(math.cos(math.radians(80.0)))
    off = sensor.SensorModel.off()
    assert all(F32(getattr(off, k)) == F32(R.OFF[k]) for k in R.FIELDS)
    c = sensor.SensorModel.constant(0.01)
    assert (c.a0, c.a1, c.a3) == (0.01, 0.0, 0.0)
    assert all(getattr(c, k) == getattr(m, k) for k in R.FIELDS if k not in ('a0', 'a1', 'a3'))
    assert sensor.SensorModel.constant(0.02, baseline=0.0).baseline == 0.0
    assert sensor.SensorModel(drop=0.1).drop == 0.1 and sensor.SensorModel(0.0).lateral_sigma == 0.0
    rec = m._replace(max_depth=4.0).record()
    assert rec.dtype == sensor.MODEL_DTYPE and rec['max_depth'] == 4.0 and rec['disparity_quantum'] == 0.125
    for bad in (dict(lateral_sigma=-1.0), dict(min_depth=5.0, max_depth=1.0), dict(baseline=math.inf), dict(cos_min=1.5),
                dict(edge_drop=-0.1), dict(drop=math.nan), dict(a1=math.inf), dict(disparity_quantum=-1.0)):
        with pytest.raises(ValueError):
            sensor.SensorModel(**bad).record()
    with pytest.raises(TypeError):
        sensor.SensorModel(sigma=1.0)
