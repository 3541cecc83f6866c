"""pycamset_amd — MI355X-native bundle-adjustment cost/Jacobian engine behind pyCamSet's
ParamHandler / optimisation_function surface.

Importing the package does not touch the GPU; the HIP extension (libpcs_hip.so) is loaded on
first use and there is no CPU fallback.
"""
from .detections import TargetDetection  # noqa: F401

__all__ = ["TargetDetection", "Engine", "parameter_covariance", "ParameterCovariance", "handlers", "function_blocks", "compiled_helpers", "pose_seeding", "device_solver", "sharding", "synthetic", "imaging", "stereo", "fusion", "sweep", "patchmatch", "volume", "raycast_views", "depth_residuals", "refine_depth_maps"]
__version__ = "0.1.0"


def __getattr__(name):
    if name == "Engine":
        from .engine import Engine
        return Engine
    if name in ("parameter_covariance", "ParameterCovariance"):
        from . import device_solver
        return getattr(device_solver, name)
    if name in ("raycast_views", "depth_residuals"):
        from . import volume
        return getattr(volume, name)
    if name == "refine_depth_maps":
        from . import patchmatch
        return patchmatch.refine_depth_maps
    if name in ("handlers", "function_blocks", "synthetic", "engine", "optimisation_handling", "sharding", "device_solver",
                "compiled_helpers", "detections", "pose_seeding", "imaging", "stereo", "fusion", "sweep", "patchmatch", "volume"):
        import importlib
        return importlib.import_module(f".{name}", __name__)
    raise AttributeError(name)
