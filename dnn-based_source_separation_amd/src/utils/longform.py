"""Window-by-window separation of long recordings: the public names of sepkernels/longform.py, where the reference's users look for utilities."""
from sepkernels.longform import separate_long, stitch

__all__ = ["separate_long", "stitch"]
