"""The colour entry points of rendering and ray casting (sgnn_amd.render, sgnn_amd.raycast)
are declared, exported by the built library and bound with the header's argument counts; each kernel exists as one
text; without a device the calls raise.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_rendercol_draw', 'sgnn_raycol_cast']


def _header():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)


def _params(src, name):
    return [p for p in re.search(r'\bint\s+%s\s*\(([^)]*)\)' % name, src).group(1).split(',') if p.strip()]


def test_colour_view_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_colour_view_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = _header()
    for prefix, names in (('sgnn_rendercol_', NAMES[:1]), ('sgnn_raycol_', NAMES[1:])):
        declared = sorted(set(re.findall(r'\b(%s[a-z0-9_]+)\s*\(' % prefix, src)))
        assert declared == names == sorted(n for n in _lib.PROTOTYPES if n.startswith(prefix))
    for name in NAMES:
        params = _params(src, name)
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert params[-1].split() == ['sgnn_stream_t', 'stream'], name
    # each takes the arguments of its depth-only entry point, then its own, then the stream
    for plain, colour, extra in (('sgnn_render_depth', 'sgnn_rendercol_draw',
                                  ['const uint8_t *vcolors', 'uint64_t *keys', 'uint8_t *rgba']),
                                 ('sgnn_raycast_cast', 'sgnn_raycol_cast', ['const uint8_t *colors', 'uint8_t *rgba'])):
        a = [' '.join(p.split()) for p in _params(src, plain)]
        b = [' '.join(p.split()) for p in _params(src, colour)]
        assert b == a[:-1] + extra + a[-1:], colour
        assert _lib.PROTOTYPES[colour][1] == _lib.PROTOTYPES[plain][1][:-1] + [_lib.c_vp] * (len(extra) + 1)
    # the depth-only entry points keep their signatures
    assert len(_lib.PROTOTYPES['sgnn_render_depth'][1]) == 17 == len(_params(src, 'sgnn_render_depth'))
    assert len(_lib.PROTOTYPES['sgnn_raycast_cast'][1]) == 18 == len(_params(src, 'sgnn_raycast_cast'))


def test_one_kernel_text_each_built_without_contraction():
    csrc = os.path.join(ROOT, 'sgnn_amd', 'csrc')
    make = open(os.path.join(csrc, 'Makefile')).read()
    for unit, kernel in (('render', 'k_render_triangles'), ('raycast', 'k_raycast')):
        assert re.search(r'^\.\./lib/%s\.o: CXXFLAGS \+= -ffp-contract=off$' % unit, make, flags=re.M)
        text = open(os.path.join(csrc, unit + '.hip')).read()
        assert len(re.findall(r'__global__[^;{]*\b%s\s*\(' % kernel, text)) == 1, kernel     # one text, COLOR or not
        assert re.search(r'template\s*<[^>]*\bbool COLOR\b[^>]*>\s*__global__[^;{]*\b%s\s*\(' % kernel, text), kernel


def test_colour_views_need_a_device(monkeypatch):
    import numpy as np
    import pytest
    import torch
    from sgnn_amd import _lib, raycast, render
    monkeypatch.setattr(torch.cuda, 'is_available', lambda: False)
    verts = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)
    faces = np.array([[0, 1, 2]], np.int32)
    k, pose = np.array([[50.0, 50.0, 15.5, 11.5]], np.float32), np.eye(4)[None]
    with pytest.raises(_lib.SgnnError):
        render.render_color(verts, faces, np.zeros((3, 3), np.uint8), k, pose, (24, 32))
    with pytest.raises(_lib.SgnnError):
        raycast.cast_color(np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4, 4), np.uint8), np.eye(4), 0.05, k, pose,
                           (24, 32), 0.15)
    with pytest.raises(_lib.SgnnError):
        raycast.cast_volume_color(object(), k, pose, (24, 32))


def test_load_ply_colors(tmp_path):
    import numpy as np
    import pytest
    from sgnn_amd import render
    rng = np.random.default_rng(0)
    verts = rng.normal(size=(7, 3)).astype(np.float32)
    cols = rng.integers(0, 256, (7, 3), dtype=np.uint8)
    faces = rng.integers(0, 7, (5, 3)).astype(np.int32)
    vdt = np.dtype([('p', '<f4', (3,)), ('c', 'u1', (3,))])
    fdt = np.dtype([('n', 'u1'), ('i', '<i4', (3,))])
    v, f = np.zeros(7, vdt), np.zeros(5, fdt)
    v['p'], v['c'], f['n'], f['i'] = verts, cols, 3, faces
    head = ('ply\nformat binary_little_endian 1.0\nelement vertex 7\nproperty float x\nproperty float y\n'
            'property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nelement face 5\n'
            'property list uchar int vertex_indices\nend_header\n')                 # marching_cubes.save_to_ply's header
    path = str(tmp_path / 'coloured.ply')
    with open(path, 'wb') as fh:
        fh.write(head.encode('ascii') + v.tobytes() + f.tobytes())
    gv, gf, gc = render.load_ply_colors(path)
    assert gc.dtype == np.uint8 and np.array_equal(gv, verts) and np.array_equal(gf, faces) and np.array_equal(gc, cols)
    two = render.load_ply(path)
    assert len(two) == 2 and np.array_equal(two[0], verts) and np.array_equal(two[1], faces)
    plain = str(tmp_path / 'plain.ply')
    with open(plain, 'wb') as fh:
        fh.write(head.replace('property uchar red\nproperty uchar green\nproperty uchar blue\n', '').encode('ascii') +
                 verts.tobytes() + f.tobytes())
    assert np.array_equal(render.load_ply(plain)[0], verts)
    with pytest.raises(ValueError, match='colours'):
        render.load_ply_colors(plain)
