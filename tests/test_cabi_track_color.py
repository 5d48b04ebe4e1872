"""The entry points of tracking with colour (sgnn_amd.track, csrc/track.hip) are declared,
exported by the built library and bound with the header's argument counts.  No GPU."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ['sgnn_track_intensity', 'sgnn_track_halve_intensity', 'sgnn_track_color_system']


def test_track_color_symbols_are_exported():
    from sgnn_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert [n for n in NAMES if not hasattr(lib, n)] == []


def test_track_color_prototypes_match_the_header():
    from sgnn_amd import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'sgnn_hip.h')).read(), flags=re.S)
    for name in NAMES:
        params = re.search(r'\b%s\s*\(([^)]*)\)' % name, src).group(1).split(',')
        res, args = _lib.PROTOTYPES[name]
        assert res is _lib.c_i32 and len(args) == len(params), name
        assert 'sgnn_stream_t stream' in params[-1] and args[-1] is _lib.c_vp, name     # the stream comes last
    # the colour system takes the geometric system's arguments and four more: two intensity stacks, two gates
    assert len(_lib.PROTOTYPES['sgnn_track_color_system'][1]) == len(_lib.PROTOTYPES['sgnn_track_system'][1]) + 4


def test_color_result_extends_track_result():
    from sgnn_amd import track
    assert track.ColorTrackResult._fields == track.TrackResult._fields + ('color_pairs', 'color_rmse')
