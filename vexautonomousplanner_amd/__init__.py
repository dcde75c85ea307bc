"""HIP-native batched trajectory planning for gfx950 (include/vap.h).  Submodules load on first use: importing the
package alone touches neither torch nor the device."""
import importlib

__all__ = ["batch", "drive", "footprint", "odometry", "plan", "search", "sensors", "timeline", "tracking"]


def __getattr__(name):
    if name in __all__:
        return importlib.import_module(f"{__name__}.{name}")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
