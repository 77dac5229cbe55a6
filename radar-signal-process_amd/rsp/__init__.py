"""rsp -- MI355X range-Doppler engine (PC -> MTD -> 0-v -> 2-D CA-CFAR), host side.

The compute lives in lib/librsp.so (HIP kernels for gfx950 behind the C ABI of
include/rsp.h); this package is the Python mirror of the reference's MATLAB interface
(rsp.matlab), parameter presets (rsp.presets), the Engine wrapper (rsp.engine), the
deterministic synthetic-echo generator (rsp.synth) and, behind the chain, the per-hit
measurement (rsp.measure), the scoring of detections against truth (rsp.score) and, in
front of it, the injection of simulated targets at a set SCR (rsp.inject).  Beside the chain,
rsp.cmap detects in the zero-velocity band the chain blanks, against a clutter map, and
rsp.width measures how wide the Doppler line of a detection's range column stands.  Behind the
measurement, rsp.track joins the estimates of successive CPIs into tracks.  rsp.oscfar is a second
detector beside the chain's cell-averaging CFAR: the ordered-statistic one.  rsp.integrate sums or
counts the planes of the last CPIs of a dwell, range walk compensated, around either detector.
rsp.fuse merges the hits of the v2 capture's stacked elevation beams per cell and estimates the
elevation from the beam amplitudes, which takes that stream to the measurement and the tracker.
"""
from . import _capi, cmap, fuse, integrate, oscfar, presets, synth, track, width  # noqa: F401
from ._capi import RspError, load_library  # noqa: F401
from .cmap import ClutterMap, band_of  # noqa: F401
from .fuse import BeamFuser  # noqa: F401
from .integrate import Integrator, walk_shifts  # noqa: F401
from .oscfar import OsCfar  # noqa: F401
from .track import Tracker  # noqa: F401
from .width import Width, ampConstrWidthEst, width_dots  # noqa: F401
from .engine import Engine, engine_for  # noqa: F401

__version__ = "0.3.0"
