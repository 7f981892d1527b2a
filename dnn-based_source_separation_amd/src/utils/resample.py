"""Sample-rate conversion: the public names of sepkernels/resample.py, where the reference's users look for utilities."""
from sepkernels.resample import Resample, StreamResampler, resample

__all__ = ["resample", "Resample", "StreamResampler"]
