"""Dynamic mixing from a device-resident corpus: the public names of sepkernels/mixing.py, where the reference's users look for utilities."""
from sepkernels.mixing import DeviceCorpus, DynamicMixer

__all__ = ["DeviceCorpus", "DynamicMixer"]
