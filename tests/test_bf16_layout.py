"""bf16 inference layout of the program executor, host side only (no GPU): the public switch and the arena queries
(sgnn_prog_arena_floats mode 3, sgnn_prog_buffer_offset infer = 2) that size and address the bf16 arena."""
import numpy as np
import pytest


def _program():
    import sgnn_amd.scn as scn
    from sgnn_amd.scn import program as P
    net = scn.Sequential().add(scn.SubmanifoldConvolution(3, 1, 16, 3, False)).add(
        scn.FullyConvolutionalNet(3, 1, [16, 32, 48], residual_blocks=True, downsample=[2, 2]))
    p = P.Program([net], 1)
    lev_n = np.array([200000 >> (3 * l) for l in range(p.n_classes)], dtype=np.int64)
    keep = np.zeros(len(p.bufs), dtype=np.int32)
    keep[p.out] = 1
    qa = (p.ops_np.ctypes.data, len(p.ops), p.bufs_np.ctypes.data, len(p.bufs), p.n_ext, lev_n.ctypes.data, p.n_classes,
          keep.ctypes.data)
    return p, lev_n, keep, qa


def test_context_manager_is_public_and_nests():
    import sgnn_amd
    from sgnn_amd.scn import program as P
    assert sgnn_amd.bf16_inference is P.bf16_inference
    assert not P.bf16_active()
    with sgnn_amd.bf16_inference():
        with sgnn_amd.bf16_inference():
            assert P.bf16_active()
        assert P.bf16_active()
    assert not P.bf16_active()
    with pytest.raises(ValueError):
        with sgnn_amd.bf16_inference():
            raise ValueError
    assert not P.bf16_active()


def test_bf16_arena_is_about_half_the_fp32_inference_arena():
    from sgnn_amd import _lib
    p, lev_n, keep, qa = _program()
    fp32 = _lib.query('sgnn_prog_arena_floats', *qa, 2)
    bf16 = _lib.query('sgnn_prog_arena_floats', *qa, 3)
    assert fp32 > 0 and 0 < bf16 <= 0.55 * fp32, (fp32, bf16)
    assert _lib.query('sgnn_prog_arena_floats', *qa, 4) == -1
    # the output (bf16 rows of 16 channels) lies inside the bf16 arena
    off = _lib.query('sgnn_prog_buffer_offset', *qa, 2, p.out)
    rows, ch = int(lev_n[p.bufs[p.out][0]]), p.bufs[p.out][1]
    assert off >= 0 and off + rows * ((ch + 7) // 8 * 8) // 2 <= bf16
    assert _lib.query('sgnn_prog_buffer_offset', *qa, 3, p.out) == -1
    # the fp32 layouts are what they were: a bf16 query in between changes nothing
    assert _lib.query('sgnn_prog_arena_floats', *qa, 2) == fp32
