"""sgnn_adam_flat, sgnn_seg_flags and sgnn_status_merge (optim.hip) against the float64 Adam step of tests/glue_ref.py.

Which set-up reaches which path:
  k_adam_flat   segments [0,5) [5,6) [7,1030) [1030,n): boundaries off multiples of 4 inside a thread's 4 elements, a
                one-element segment, element 6 in no segment; n = 1031 and 4099 (n % 4 = 3: the ragged last thread);
                n = 1024 x 1024 + 3 exceeds the launch's 1024 blocks x 256 threads x 4 elements: a second grid trip.
                Activity: by cnt, by flag, by flag against a contradicting cnt, by neither (always on).
                Status with the overflow bit: the early return, nothing changes.
  k_adam_steps  active counters + 1 exactly, inactive and overflowed ones bit-identical.
  k_seg_flags, k_status_merge  one form each.

Bars (one step from glue_ref.adam_state):
  m, v within 4 ulp of the float64 step.
  |p - p64| <= 2^-24 |p64| + 32 x 2^-24 x U, U = lr (|m0| + |g'|) / (bc1 (sqrt(v64) / sqrt(bc2) + eps)).
  Roundings on the way from the inputs to the update, as the kernel is written (a contraction only removes some):
  g' = g * scale (1), + p * wd (2); m: g' - m (1), * (1 - b1) (1), + m (1); v: b2 * v (1), (1 - b2) * g' (1), * g' (1),
  sum (1); bc1 and bc2 from double to float (2), sqrtf(bc2) (1); lr / bc1 (1); sqrtf(v) (1), / bc2s (1), + eps (1);
  step * m (1), / denom (1): 20, each at most 2^-24 relative to a term no larger than its absolute-value counterpart
  in U; the final subtraction is the 2^-24 |p64| term.  32 is the ceiling over those 20.
  With SGNN_ADAM_RATIOS set to a file name every case appends its largest ratio |p - p64| / bound there
  (profiles/adam_fp64_ratios.txt holds an MI355X run: 0.91 .. 0.998, and 0 where
  nothing is updated.  The ratios sit just below 1 because storing p in
  float32 alone costs up to half an ulp, which is 2^-24 |p64| for a mantissa near 1, the whole first term of the bound;
  the update is small against p, so the 32 x 2^-24 x U term hardly enters.  m and v stay within 2.1 and 2.9 ulp.)"""
import itertools
import os

import numpy as np
import pytest

import glue_ref as R

pytestmark = pytest.mark.gpu

LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-8
OVERFLOW = R.STATUS_OVERFLOW
# how each of the four segments learns whether it was reached: (cnt, flag) values, None = no pointer
ACTIVITY = {
    'cnt': [(5, None), (0, None), (5, None), (0, None)],
    'flag': [(None, 0.0), (None, 1.0), (None, 0.0), (None, 1.0)],
    'flag_over_cnt': [(0, 1.0), (5, 0.0), (5, 0.0), (0, 1.0)],
    'neither': [(None, None)] * 4,
    'mixed': [(5, None), (None, 0.0), (None, None), (0, 1.0)],
}


def L():
    from sgnn_amd import _lib
    return _lib


def _record(what, ratio):
    path = os.environ.get('SGNN_ADAM_RATIOS')
    if path:
        with open(path, 'a') as f:
            f.write('%-72s %.4f\n' % (what, ratio))


def _step(n, activity, steps, wd, scale, status, what):
    segs = R.adam_segments(n)
    p, g, m, v = R.adam_state(what, n)
    dp, dg, dm, dv = R.dev_in(p), R.dev_in(g), R.dev_in(m), R.dev_in(v)
    lr = R.dev_in(np.array([LR], np.float32))
    cnts = [None if c is None else R.dev_in(np.array([c], np.int64)) for c, _ in activity]
    flags = [None if f is None else R.dev_in(np.array([f], np.float32)) for _, f in activity]
    ctr = [R.dev_in(np.array([s], np.float32)) for s in steps]
    st = None if status is None else R.dev_in(np.array([status], np.int32))
    seg = np.array([[b, e, 0 if c is None else c.ptr, 0 if f is None else f.ptr, k.ptr]
                    for (b, e), c, f, k in zip(segs, cnts, flags, ctr)], np.int64)
    L().call('sgnn_adam_flat', dp.ptr, dg.ptr, dm.ptr, dv.ptr, n, seg.ctypes.data, len(segs), lr.ptr, B1, B2, EPS, wd, scale,
             None if st is None else st.ptr)
    active = [R.segment_active(c, f) for c, f in activity]
    ref = R.adam_step(p, g, m, v, segs, steps, active, LR, B1, B2, EPS, wd, scale, status)
    got = [b.check('%s: %s' % (what, nm)) for b, nm in zip((dp, dm, dv), 'pmv')]
    R.assert_same_bits(dg.check(what + ': g'), g, what + ': the gradient is read-only')
    counters = [float(k.check(what)[0]) for k in ctr]
    assert counters == ref[3], '%s: step counters %s, expected %s' % (what, counters, ref[3])
    blocked = R.status_blocks(status)
    assert ref[4].sum() == (0 if blocked else sum(e - b for (b, e), a in zip(segs, active) if a))
    assert not ref[4][6]                                              # element 6 belongs to no segment
    if st is not None:
        assert int(st.check(what)[0]) == status
    ratio = R.assert_adam(got[0], got[1], got[2], ref, (p, m, v), what)
    _record(what, ratio)


@pytest.mark.parametrize('n', [1031, 4099])
@pytest.mark.parametrize('rule', list(ACTIVITY))
def test_adam_step(n, rule):
    k = 0
    for wd, scale in itertools.product((0.0, 1e-3), (1.0, 0.125)):
        for status in (None, 0, R.STATUS_DUPLICATE):
            steps = [R.ADAM_STEPS[(k + t) % 5] for t in range(4)]
            _step(n, ACTIVITY[rule], steps, wd, scale, status,
                  'adam n=%d %s wd=%g scale=%g status=%s steps=%s' % (n, rule, wd, scale, status, steps))
            k += 1


@pytest.mark.parametrize('rule', ['neither', 'mixed'])
def test_adam_overflowed_step_changes_nothing(rule):
    for n, status in ((1031, OVERFLOW), (4099, OVERFLOW | R.STATUS_DUPLICATE)):
        _step(n, ACTIVITY[rule], [0, 9, 999, 100000], 1e-3, 0.125, status, 'adam n=%d %s overflowed' % (n, rule))


def test_adam_second_grid_trip():
    n = 1024 * 1024 + 3
    _step(n, ACTIVITY['neither'], [100000, 0, 1, 9], 1e-3, 0.125, 0, 'adam n=%d neither wd=0.001 scale=0.125' % n)
    _step(n, ACTIVITY['mixed'], [1, 9, 999, 0], 0.0, 1.0, None, 'adam n=%d mixed wd=0 scale=1' % n)


def test_seg_flags():
    for nseg in (1, 7):
        for status in (None, 0, R.STATUS_DUPLICATE, OVERFLOW, OVERFLOW | R.STATUS_COORD_RANGE):
            vals = [(None, 3, 0, 1, None, 0, 7)[t] for t in range(nseg)]
            cnts = [None if c is None else R.dev_in(np.array([c], np.int64)) for c in vals]
            ptrs = np.array([0 if c is None else c.ptr for c in cnts] + [0], np.int64)
            flags = R.dev_out((8,), np.float32)
            st = None if status is None else R.dev_in(np.array([status], np.int32))
            L().call('sgnn_seg_flags', ptrs.ctypes.data, nseg, flags.ptr, None if st is None else st.ptr)
            what = 'seg_flags nseg=%d status=%s' % (nseg, status)
            written = np.arange(8) < nseg
            if status is not None:
                written[7] = True
            got = flags.check(what, untouched=~written)
            want = [1.0 if (c is None or c > 0) else 0.0 for c in vals]
            assert got[:nseg].tolist() == want, '%s: %s' % (what, got)
            if status is not None:
                assert got[7] == (1.0 if status & OVERFLOW else 0.0), '%s: overflow slot %s' % (what, got[7])
                assert int(st.check(what)[0]) == status


def test_status_merge():
    for flag in (0.0, 1.0, 2.0):
        for preset in (0, R.STATUS_DUPLICATE, R.STATUS_COORD_RANGE | R.STATUS_DUPLICATE, OVERFLOW):
            f, st = R.dev_in(np.array([flag], np.float32)), R.dev_in(np.array([preset], np.int32))
            L().call('sgnn_status_merge', f.ptr, st.ptr)
            want = preset | (OVERFLOW if flag > 0 else 0)
            assert int(st.check('status_merge')[0]) == want, (flag, preset)
