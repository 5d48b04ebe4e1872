"""sgnn_amd — MI355X-native sparse generative 3D convolution hot path for SG-NN.

Package contents (only what the hot path of SURVEY.md §8 needs):
  csrc/        hand-written gfx950 HIP kernels + the C ABI (include/sgnn_hip.h)
  _lib.py      ctypes binding (fails loudly without the .so / a GPU; no CPU fallback)
  scn/         `sparseconvnet`-compatible operator surface (torch/model.py:7)
  model.py     GenModel counterpart (torch/model.py:276) on the fused device-side glue
  loss.py      compute_targets / compute_loss (torch/loss.py:15-199)
  train.py     one training step + data-parallel gradient all-reduce (torch/train.py:245-268)
  synth.py     synthetic TSDF blocks in the layout scene_dataloader.collate emits
  track.py     depth frames tracked against a TSDF volume: poses for fusion
  register.py  point sets and volumes registered against a TSDF volume: transforms for regrid.merge (section R)
  upright.py   the gravity-aligned room frame of a scan volume: the transform for regrid.grid_for (section S)
  sensor.py    a depth sensor simulated on rendered frames: noise, disparity steps, shadow, ragged edges (section V)
  smooth.py    triangle meshes faired: adjacency, Laplacian / Taubin smoothing, normals, denoising (section Y)
  raytrace.py  arbitrary rays against a triangle mesh: closest hits, scanner sweeps for points, visibility (section W)
  cloud.py     point-cloud neighbourhoods: exact kNN and radius search, normals, outlier filters, voxel thinning (section Z)
"""
__version__ = '0.1.0'


def __getattr__(name):
    # sgnn_amd.bf16_inference: the bf16 inference mode of the program executor (scn/program.py); resolved lazily so that
    # importing the package stays free of torch / the native library
    if name == 'bf16_inference':
        from .scn.program import bf16_inference
        return bf16_inference
    if name in ('track', 'register', 'upright', 'sensor', 'raytrace', 'cloud'):   # sgnn_amd.track / .register / .upright / .sensor / .raytrace / .cloud without an import statement of their own, as lazily as the above
        import importlib
        return importlib.import_module('.' + name, __name__)
    raise AttributeError(name)
